// engine_pipeline.hip -- the host-to-host entry points (include/raft_hip.h raft_hip_run_host_grouped ... raft_hip_run_pipelined):
// page-locked host columns in, every output in host memory out, with upload / pass / download of consecutive read ranges overlapped,
// over one context or several (one per GPU), and the host-routed path for streams that are not a handful of sorted runs.  Everything
// here is host code around the passes of engine.hip; the arithmetic of the chunk plan is pipeline_plan.hpp.
#include "engine_ctx.hpp"
#include "pipeline_plan.hpp"

#include <memory>

static_assert(kPlanSeg == kMaxSeg, "a chunk keeps one piece per sorted run the fast path accepts");

extern "C" {

namespace {

constexpr int kOnePiece = -1;           // a phase's answer: nothing the caller sees was done, the job goes to the one-piece pass

#define PHASE(expr)                                              \
    do {                                                         \
        const int rc_ = (expr);                                  \
        if (rc_ == kOnePiece) return one_piece(P);               \
        if (rc_ != RAFT_HIP_OK) return rc_;                      \
    } while (0)

// what a pass reports about the data (or about a record outside the chunk it was cut into): the one-piece pass reports it properly
bool is_data_error(int rc) { return rc == RAFT_HIP_ERR_READ_ID || rc == RAFT_HIP_ERR_COORD || rc == RAFT_HIP_ERR_FRAGMENT || rc == RAFT_HIP_ERR_PARAM; }

// bytes per window of the coverage's transfer encoding (or the delta4 code) for a caller's cov_width
int transfer_width(int cov_width) { return cov_width == kCovDelta4 ? kCovDelta4 : (cov_width == 2 ? 2 : 1); }

// the context's page-locked staging block holds `bytes` (+ headroom when it has to be made anew)
int ensure_stage(raft_hip_ctx *c, size_t bytes, size_t headroom = 0)
{
    if (bytes <= c->h_stage_cap) return RAFT_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    c->h_stage = nullptr; c->h_stage_cap = 0;
    HIP_TRY(c, hipHostMalloc(&c->h_stage, bytes + headroom, hipHostMallocDefault));
    c->h_stage_cap = bytes + headroom;
    return RAFT_HIP_OK;
}

// A context set up for one internal call: parameters (if any) and output width for the call, both put back when the scope ends;
// unless the caller is to fetch the pass, `ran` / `finished` are cleared then -- the context holds no pass of the caller's.
struct SetupGuard {
    raft_hip_ctx *c;
    const raft_hip_params keep_prm;
    const int keep_width;
    const bool had_prm, keeps_pass;
    SetupGuard(raft_hip_ctx *c_, const raft_hip_params *prm, int width, bool keeps_pass_ = false)
        : c(c_), keep_prm(c_->prm), keep_width(c_->out_width), had_prm(prm != nullptr), keeps_pass(keeps_pass_)
    {
        if (prm) apply_params(c, prm);
        c->out_width = width;
    }
    SetupGuard(const SetupGuard &) = delete;
    ~SetupGuard()
    {
        c->out_width = keep_width;
        if (had_prm) apply_params(c, &keep_prm);
        if (!keeps_pass) { c->ran = false; c->finished = false; }
    }
};

// A chain of tickets: the holder of ticket k waits until a counter has reached k, takes its turn under the mutex and hands
// on k + 1.  The first failure (or `also_stop`) ends every wait.
struct TicketChain {
    std::mutex mu;
    std::condition_variable cv;
    int error = RAFT_HIP_OK;                        // first failure; everybody stops at the next check
    std::string error_text;
    const std::atomic<bool> *also_stop = nullptr;
    bool stopped() const { return error != RAFT_HIP_OK || (also_stop && also_stop->load()); }   // (mu held)
    // the lock comes back held for the turn, or released when the chain has stopped
    std::unique_lock<std::mutex> await(const int &counter, int ticket)
    {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return counter == ticket || stopped(); });
        if (stopped()) g.unlock();
        return g;
    }
    void hand_on(int &counter, int ticket) { counter = ticket + 1; cv.notify_all(); }      // (mu held)
    bool fail(int code, const std::string &text)    // true: this is the chain's first failure
    {
        std::lock_guard<std::mutex> g(mu);
        const bool first = error == RAFT_HIP_OK;
        if (first) { error = code; error_text = text; }
        cv.notify_all();
        return first;
    }
    bool wake() { std::lock_guard<std::mutex> g(mu); cv.notify_all(); return stopped(); }
};

} // namespace

static int run_host_grouped_impl(raft_hip_ctx *c, const HostInput &in, int64_t n_bins)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    const int32_t n_reads = in.n_reads, n_runs = in.n_runs;
    const int64_t n_rec = in.n_rec;
    if (n_reads < 0 || n_rec < 0 || n_runs < 1 || n_runs > kMaxRuns || !in.rec_offset) return RAFT_HIP_ERR_PARAM;
    if (n_reads > 0 && !in.read_len) return RAFT_HIP_ERR_PARAM;
    if (n_rec > 0 && (!in.qs || !in.qe) && !in.win) return RAFT_HIP_ERR_PARAM;
    if (c->prm.symmetric_mode != 1) return RAFT_HIP_ERR_PARAM;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t n_off = (size_t)n_runs * ((size_t)n_reads + 1);
    HIP_TRY(c, c->in_len.ensure((size_t)std::max<long long>(n_reads, 1) * 4));
    HIP_TRY(c, c->in_off.ensure(n_off * 8));
    if (n_reads) HIP_TRY(c, hipMemcpyAsync(c->in_len.p, in.read_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->in_off.p, in.rec_offset, n_off * 8, hipMemcpyHostToDevice, st));
    const void *src[3] = {nullptr, in.win ? (const void *)in.win : (const void *)in.qs, in.qe};
    for (int k = 1; k < (in.win ? 2 : 3); ++k) {
        HIP_TRY(c, c->in_col[k].ensure((size_t)std::max<long long>(n_rec, 1) * 4));
        if (n_rec) HIP_TRY(c, hipMemcpyAsync(c->in_col[k].p, src[k], (size_t)n_rec * 4, hipMemcpyHostToDevice, st));
    }
    if (n_bins < 0) n_bins = count_windows(in.read_len, n_reads, WindowDiv(c->prm.reso));      // (while the copies run)
    if (in.win)
        return run_grouped(c, n_reads, c->in_len.as<int32_t>(), n_rec, n_runs, c->in_off.as<int64_t>(), nullptr, nullptr, nullptr, nullptr, n_bins,
                           c->in_col[1].as<uint32_t>());
    return run_grouped(c, n_reads, c->in_len.as<int32_t>(), n_rec, n_runs, c->in_off.as<int64_t>(), nullptr, nullptr,
                       c->in_col[1].as<int32_t>(), c->in_col[2].as<int32_t>(), n_bins);
}

static HostInput grouped_input(int32_t n_reads, const int32_t *read_len, int64_t n_rec, int32_t n_runs, const int64_t *rec_offset, const int32_t *qs,
                               const int32_t *qe, const uint32_t *win)
{
    HostInput in;
    in.n_reads = n_reads; in.read_len = read_len; in.n_rec = n_rec;
    in.qs = qs; in.qe = qe;
    in.n_runs = n_runs; in.rec_offset = rec_offset; in.win = win;
    return in;
}

int raft_hip_run_host_grouped(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, int32_t n_runs,
                              const int64_t *rec_offset, const int32_t *qs, const int32_t *qe, int64_t n_bins)
{
    return run_host_grouped_impl(c, grouped_input(n_reads, read_len, n_rec, n_runs, rec_offset, qs, qe, nullptr), n_bins);
}

int raft_hip_run_host_windows(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, int32_t n_runs,
                              const int64_t *rec_offset, const uint32_t *win, int64_t n_bins)
{
    if (n_rec > 0 && !win) return RAFT_HIP_ERR_PARAM;
    static const uint32_t none = 0;
    return run_host_grouped_impl(c, grouped_input(n_reads, read_len, n_rec, n_runs, rec_offset, nullptr, nullptr, win ? win : &none), n_bins);
}

// the whole job as one pass on one context, every output fetched into the caller's arrays
static int run_monolithic_to_host(raft_hip_ctx *c, const HostInput &in, raft_hip_host_outputs *o, raft_hip_summary *summary)
{
    const int width = transfer_width(o->cov_width);
    raft_hip_summary s{};
    int rc;
    {
        SetupGuard setup(c, nullptr, width, true);            // the pass writes the encoding the caller takes
        rc = in.rec_offset ? run_host_grouped_impl(c, in, -1)
                           : raft_hip_run_host(c, in.n_reads, in.read_len, in.n_rec, in.qid, in.qs, in.qe, in.tid, in.ts, in.te);
        if (rc == RAFT_HIP_OK) rc = raft_hip_finish(c, &s);
    }
    s.n_devices_used = 1;
    if (summary) *summary = s;
    if (rc != RAFT_HIP_OK) return rc;
    if (s.n_bins > o->cov8_cap || s.n_repeats > o->rep_cap || s.n_fragments > o->frag_cap) return RAFT_HIP_ERR_TOO_LARGE;
    int64_t n_exc = 0;
    if (width == kCovDelta4 && (s.n_bins + kD4Block - 1) / kD4Block > o->anchor_cap) return RAFT_HIP_ERR_TOO_LARGE;
    rc = fetch_packed_impl(c, width, o->cov_offset, o->cov8, width == kCovDelta4 ? o->cov_anchor : nullptr, o->exc_cap, o->exc_index, o->exc_value, &n_exc,
                           o->rep_offset, o->rep_s, o->rep_e, o->frag_offset, nullptr, o->frag_begin, o->frag_end);
    o->n_exc = n_exc;
    return rc;
}

namespace {

constexpr int kLanes = 4;

int prepare_lanes(raft_hip_ctx *c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    // Copies get streams of their own priority levels.  The runtime multiplexes streams onto a few hardware queues per
    // priority level, and a copy holds its queue for its whole duration: on a queue shared with a lane's compute stream
    // the kernels of one chunk sat behind the uploads of the next two (measured: 12 ms of a 0.4 ms pass).
    if (!c->up_stream) {
        int lo_p = 0, hi_p = 0;                      // numerically lowest = highest priority
        HIP_TRY(c, hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));
        HIP_TRY(c, hipStreamCreateWithPriority(&c->up_stream, hipStreamNonBlocking, hi_p));
        HIP_TRY(c, hipStreamCreateWithPriority(&c->down_stream, hipStreamNonBlocking, lo_p));
    }
    while ((int)c->lanes.size() < kLanes) {
        raft_hip_ctx *l = nullptr;
        const int rc = raft_hip_create(c->device, &c->prm, &l);
        if (rc != RAFT_HIP_OK) return rc;
        c->lanes.push_back(l);
        hipEvent_t e, d;
        HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->lane_up_ev.push_back(e);
        HIP_TRY(c, hipEventCreateWithFlags(&d, hipEventDisableTiming));
        c->lane_down_ev.push_back(d);
    }
    for (raft_hip_ctx *l : c->lanes) {
        apply_params(l, &c->prm);
        l->tile_q = c->tile_q; l->force_bucket = 0;
        l->is_lane = true;
        l->emit_cuts = false;                         // (raft_hip_host_outputs holds no cut points)
    }
    return RAFT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Host-routed jobs for record streams that are NOT a handful of runs sorted by query id (a shuffled PAF, a non-symmetric
// one, more than four concatenated files): SURVEY.md §8(e)'s host-routed mode in its general form.  create_pileup's
// bucketing (chop.hpp:155-169: every record into its query's bucket and, while the PAF is not symmetric, into its
// target's) is done by the host's threads as a counting sort by read id -- counts, offsets, scatter -- which leaves the
// intervals grouped by read: consecutive read ranges are then contiguous slices, each a sorted run of its own, and go
// to the contexts (devices) in turn as one-piece passes of the sorted-segment path; a chain of tickets hands each chunk
// the sizes of the chunks before it.  This is also what lifts the 2^29-records-per-pass limit for such inputs.
// ---------------------------------------------------------------------------------------------------------------------
struct Routed {
    const HostInput &in;
    raft_hip_host_outputs *o;
    int mode = 0, sym = 0, T = 1, cov_width = 1;
    std::vector<long long> pre;                      // intervals before every read
    std::unique_ptr<int32_t[]> cur, b_rid, b_s, b_e; // the intervals grouped by read
    long long total = 0;
    std::vector<int32_t> bound;                      // chunk k: reads [bound[k], bound[k + 1])
    int n_ch = 0, n_job = 0;
    TicketChain chain;                               // publishes the sizes in chunk order
    int published = 0;
    bool data_error = false;                         // the first failure is one the one-piece pass reports properly
    long long base_bins = 0, base_rep = 0, base_frag = 0, base_exc = 0;
    raft_hip_summary tot{};
    Routed(const HostInput &in_, raft_hip_host_outputs *o_) : in(in_), o(o_) {}
    void fail(raft_hip_ctx *jc, int code, bool data) { if (chain.fail(code, jc->last_error)) data_error = data; }
};

// ids in range?  the mirror of record 0 (chop.hpp:171-184) when the caller did not say.  The first record out of range, or -1.
long long routed_check_ids(Routed &R)
{
    const HostInput &in = R.in;
    const int T = R.T, mode = R.mode;
    const int32_t *qid = in.qid, *qs = in.qs, *qe = in.qe, *tid = in.tid, *ts = in.ts, *te = in.te;
    std::vector<long long> bad((size_t)T, -1);
    std::vector<int> mirror((size_t)T, 0);
    host_parallel(T, [&](int t) {
        const long long lo = in.n_rec * t / T, hi = in.n_rec * (t + 1) / T;
        const bool detect = mode < 0 && in.n_rec > 0;
        const int32_t q0 = detect ? qid[0] : 0, t0 = detect ? tid[0] : 0, qs0 = detect ? qs[0] : 0, qe0 = detect ? qe[0] : 0, ts0 = detect ? ts[0] : 0,
                      te0 = detect ? te[0] : 0;
        for (long long i = lo; i < hi; ++i) {
            const bool okq = (uint32_t)qid[i] < (uint32_t)in.n_reads, okt = mode == 1 || (uint32_t)tid[i] < (uint32_t)in.n_reads;
            if (!(okq && okt)) { if (bad[(size_t)t] < 0) bad[(size_t)t] = i; continue; }
            if (detect && i > 0 && qid[i] == t0 && tid[i] == q0 && ts[i] == qs0 && te[i] == qe0 && qs[i] == ts0 && qe[i] == te0) mirror[(size_t)t] = 1;
        }
    });
    for (int t = 0; t < T; ++t)
        if (bad[(size_t)t] >= 0) return bad[(size_t)t];
    R.sym = mode == 1 ? 1 : 0;
    if (mode < 0) for (int t = 0; t < T; ++t) R.sym |= mirror[(size_t)t];
    return -1;
}

// counting sort by read id on the host, first half: counts and offsets (symmetric: query sides; else also target sides of
// records whose two reads differ -- bucket.hpp's multiset)
int routed_count(Routed &R)
{
    const HostInput &in = R.in;
    const int T = R.T, sym = R.sym;
    try {
        R.pre.assign((size_t)in.n_reads + 1, 0);
        R.cur.reset(new int32_t[(size_t)in.n_reads + 1]());
    } catch (const std::bad_alloc &) { return RAFT_HIP_ERR_NOMEM; }
    int32_t *cur = R.cur.get();
    host_parallel(T, [&](int t) {
        const long long lo = in.n_rec * t / T, hi = in.n_rec * (t + 1) / T;
        for (long long i = lo; i < hi; ++i) {
            __atomic_fetch_add(&cur[(size_t)in.qid[i]], 1, __ATOMIC_RELAXED);
            if (!sym && in.tid[i] != in.qid[i]) __atomic_fetch_add(&cur[(size_t)in.tid[i]], 1, __ATOMIC_RELAXED);
        }
    });
    for (int32_t r = 0; r < in.n_reads; ++r) {
        if (cur[(size_t)r] < 0) return RAFT_HIP_ERR_TOO_LARGE;          // (2^31 intervals on one read)
        R.pre[(size_t)r + 1] = R.pre[(size_t)r] + cur[(size_t)r];
        cur[(size_t)r] = 0;
    }
    R.total = R.pre[(size_t)in.n_reads];
    return RAFT_HIP_OK;
}

// ... second half: every side to its read's place
int routed_scatter(Routed &R)
{
    const HostInput &in = R.in;
    const int T = R.T, sym = R.sym;
    const size_t n = (size_t)std::max(R.total, 1LL);
    try {
        R.b_rid.reset(new int32_t[n]); R.b_s.reset(new int32_t[n]); R.b_e.reset(new int32_t[n]);
    } catch (const std::bad_alloc &) { return RAFT_HIP_ERR_NOMEM; }
    int32_t *cur = R.cur.get(), *b_rid = R.b_rid.get(), *b_s = R.b_s.get(), *b_e = R.b_e.get();
    const long long *pre = R.pre.data();
    host_parallel(T, [&](int t) {
        const long long lo = in.n_rec * t / T, hi = in.n_rec * (t + 1) / T;
        auto put = [&](int32_t r, int32_t s0, int32_t e0) {
            const long long d = pre[(size_t)r] + __atomic_fetch_add(&cur[(size_t)r], 1, __ATOMIC_RELAXED);
            b_rid[(size_t)d] = r; b_s[(size_t)d] = s0; b_e[(size_t)d] = e0;
        };
        for (long long i = lo; i < hi; ++i) {
            put(in.qid[i], in.qs[i], in.qe[i]);
            if (!sym && in.tid[i] != in.qid[i]) put(in.tid[i], in.ts[i], in.te[i]);
        }
    });
    R.cur.reset();
    return RAFT_HIP_OK;
}

// plan: consecutive read ranges of near-equal interval counts, each far below the per-pass limit
int routed_bounds(Routed &R, int32_t n_chunks, int32_t n_ctx)
{
    const int32_t n_reads = R.in.n_reads;
    const long long per_pass = 1LL << 27;
    long long want = std::max<long long>(std::max<long long>(n_chunks, n_ctx), (R.total + per_pass - 1) / per_pass);
    want = std::max<long long>(1, std::min<long long>(want, std::max(n_reads, 1)));
    R.bound.assign(1, 0);
    for (long long k = 1; k < want; ++k) {
        const long long target = R.total * k / want;
        const int32_t r = (int32_t)(std::lower_bound(R.pre.begin(), R.pre.end(), target) - R.pre.begin());
        if (r > R.bound.back() && r < n_reads) R.bound.push_back(r);
    }
    R.bound.push_back(n_reads);
    R.n_ch = (int)R.bound.size() - 1;
    for (int k = 0; k < R.n_ch; ++k)
        if (R.pre[(size_t)R.bound[(size_t)k + 1]] - R.pre[(size_t)R.bound[(size_t)k]] >= (1LL << 29)) return RAFT_HIP_ERR_TOO_LARGE;   // (one read's pile alone)
    R.n_job = std::min(n_ctx, std::max(R.n_ch, 1));
    return RAFT_HIP_OK;
}

// chunk k on context jc: staging, the pass, its place from the chain, the fetch.  false: the job stops here.
bool routed_chunk(Routed &R, raft_hip_ctx *jc, int k)
{
    raft_hip_host_outputs *o = R.o;
    const int cov_width = R.cov_width;
    const int32_t r0 = R.bound[(size_t)k], r1 = R.bound[(size_t)k + 1], nr = r1 - r0;
    const long long i0 = R.pre[(size_t)r0], n_iv = R.pre[(size_t)r1] - i0;
    raft_hip_summary s{};
    hipError_t e = hipSetDevice(jc->device);
    if (e == hipSuccess) e = jc->in_len.ensure((size_t)std::max(nr, 1) * 4);
    for (int col = 0; col < 3 && e == hipSuccess; ++col) e = jc->in_col[col].ensure((size_t)std::max<long long>(n_iv, 1) * 4);
    if (e == hipSuccess && nr) e = hipMemcpyAsync(jc->in_len.p, R.in.read_len + r0, (size_t)nr * 4, hipMemcpyHostToDevice, jc->stream);
    const int32_t *src[3] = {R.b_rid.get() + i0, R.b_s.get() + i0, R.b_e.get() + i0};
    for (int col = 0; col < 3 && e == hipSuccess && n_iv; ++col)
        e = hipMemcpyAsync(jc->in_col[col].p, src[col], (size_t)n_iv * 4, hipMemcpyHostToDevice, jc->stream);
    if (e != hipSuccess) { R.fail(jc, fail_hip(jc, e, "run_routed: staging"), false); return false; }
    if (n_iv > 0 && r0 != 0)
        launch_rebase_ids(jc->stream, jc->in_col[0].as<int32_t>(), n_iv, r0);
    int rc = raft_hip_run_device(jc, nr, jc->in_len.as<int32_t>(), n_iv, jc->in_col[0].as<int32_t>(), jc->in_col[1].as<int32_t>(),
                                 jc->in_col[2].as<int32_t>(), nullptr, nullptr, nullptr);
    if (rc == RAFT_HIP_OK) rc = raft_hip_finish(jc, &s);
    // (a data error's index counts the routed intervals, not the caller's records: the one-piece pass reports it
    // properly when the input is small enough for one)
    if (rc != RAFT_HIP_OK) { R.fail(jc, rc, is_data_error(rc)); return false; }
    long long b_bins, b_rep, b_frag, b_exc;
    {
        auto turn = R.chain.await(R.published, k);
        if (!turn.owns_lock()) return false;
        b_bins = R.base_bins; b_rep = R.base_rep; b_frag = R.base_frag; b_exc = R.base_exc;
    }
    // sizes of the encoding's exception list are known only after it has been made (raft_hip_fetch_packed_w's size query)
    int64_t n_exc = 0;
    rc = raft_hip_fetch_packed_w(jc, cov_width, nullptr, nullptr, 0, nullptr, nullptr, &n_exc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    const bool fits = rc == RAFT_HIP_OK && b_bins + s.n_bins <= o->cov8_cap && b_rep + s.n_repeats <= o->rep_cap &&
                      b_frag + s.n_fragments <= o->frag_cap;
    const bool exc_fits = b_exc + n_exc <= o->exc_cap;
    if (rc == RAFT_HIP_OK && !fits) { jc->last_error = "host output capacity (coverage / repeats / fragments)"; rc = RAFT_HIP_ERR_TOO_LARGE; }
    if (rc == RAFT_HIP_OK)   // (a list that no longer fits is counted, not fetched: the call ends with TOO_LARGE and the job's total)
        rc = raft_hip_fetch_packed_w(jc, cov_width, o->cov_offset + r0, o->cov8 ? o->cov8 + b_bins * cov_width : nullptr, n_exc,
                                     (exc_fits && o->exc_index) ? o->exc_index + b_exc : nullptr, (exc_fits && o->exc_value) ? o->exc_value + b_exc : nullptr,
                                     &n_exc, o->rep_offset + r0, o->rep_s ? o->rep_s + b_rep : nullptr, o->rep_e ? o->rep_e + b_rep : nullptr,
                                     o->frag_offset + r0, nullptr, o->frag_begin ? o->frag_begin + b_frag : nullptr,
                                     o->frag_end ? o->frag_end + b_frag : nullptr);
    if (rc != RAFT_HIP_OK) { R.fail(jc, rc, false); return false; }
    // (the fetch wrote nr + 1 offsets counting from this chunk's first entry: the closing one is the next chunk's first)
    for (int32_t r = 0; r < nr + (k == R.n_ch - 1 ? 1 : 0); ++r) {
        o->cov_offset[r0 + r] += b_bins; o->rep_offset[r0 + r] += b_rep; o->frag_offset[r0 + r] += b_frag;
    }
    if (exc_fits && o->exc_index) for (int64_t i = 0; i < n_exc; ++i) o->exc_index[b_exc + i] += b_bins;
    std::lock_guard<std::mutex> g(R.chain.mu);
    raft_hip_summary &tot = R.tot;
    R.base_bins += s.n_bins; R.base_rep += s.n_repeats; R.base_frag += s.n_fragments; R.base_exc += n_exc;
    tot.n_bins += s.n_bins; tot.n_repeats += s.n_repeats; tot.n_fragments += s.n_fragments; tot.n_cuts += s.n_cuts;
    tot.n_intervals += s.n_intervals; tot.total_coverage += s.total_coverage; tot.total_repeat_length += s.total_repeat_length;
    tot.total_read_length += s.total_read_length; tot.flags |= s.flags & RAFT_HIP_SUM_GRADED_RANGES;
    R.chain.hand_on(R.published, k);
    return true;
}

} // namespace

// *fallback = true: nothing was done and the caller should take the one-piece pass (which reports data errors exactly).
static int run_routed(raft_hip_ctx *const *ctxs, int32_t n_ctx, const HostInput &in, int32_t n_chunks, raft_hip_host_outputs *o, raft_hip_summary *summary,
                      bool *fallback)
{
    raft_hip_ctx *c = ctxs[0];
    *fallback = false;
    Routed R(in, o);
    R.mode = c->prm.symmetric_mode;
    if (R.mode != 1 && (!in.tid || !in.ts || !in.te)) return RAFT_HIP_ERR_PARAM;
    const bool one_pass_possible = in.n_rec < (1LL << 29);
    R.cov_width = transfer_width(o->cov_width);           // (never delta4 here: run_multi_impl keeps that in one piece)
    R.T = (int)std::min<long long>(std::max(1u, std::thread::hardware_concurrency()), 32);
    if (in.n_rec < (1 << 18)) R.T = 1;
    const long long bad = routed_check_ids(R);
    if (bad >= 0) {
        if (one_pass_possible) { *fallback = true; return RAFT_HIP_OK; }
        raft_hip_summary s{};
        s.n_reads = in.n_reads; s.n_records = in.n_rec; s.high_cov = c->high_cov; s.error_index = bad;
        if (summary) *summary = s;
        return RAFT_HIP_ERR_READ_ID;
    }
    int rc = routed_count(R);
    if (rc == RAFT_HIP_OK) rc = routed_scatter(R);
    if (rc == RAFT_HIP_OK) rc = routed_bounds(R, n_chunks, n_ctx);
    if (rc != RAFT_HIP_OK) return rc;
    const int n_job = R.n_job;
    raft_hip_params prm1 = c->prm;
    prm1.symmetric_mode = 1;                              // the routed intervals ARE the multiset to pile up: query-side records
    std::vector<std::unique_ptr<SetupGuard>> setup;
    for (int d = 0; d < n_job; ++d) {
        setup.push_back(std::make_unique<SetupGuard>(ctxs[d], &prm1, R.cov_width));
        ctxs[d]->tile_q = c->tile_q;
    }
    raft_hip_summary &tot = R.tot;
    tot.n_reads = in.n_reads; tot.symmetric = R.sym; tot.high_cov = c->high_cov; tot.n_records = in.n_rec; tot.error_index = -1;
    tot.interval_path = 0; tot.n_segments = 1; tot.n_devices_used = n_job;
    // chunk k runs on context k % n_job
    auto job_main = [&](int d) {
        for (int k = d; k < R.n_ch; k += n_job) {
            if (R.chain.wake()) break;
            if (!routed_chunk(R, ctxs[d], k)) break;
        }
    };
    {
        std::vector<std::thread> th;
        for (int d = 1; d < n_job; ++d) th.emplace_back([&, d] { job_main(d); });
        job_main(0);
        for (auto &t : th) t.join();
    }
    setup.clear();
    (void)hipSetDevice(c->device);
    if (R.chain.error != RAFT_HIP_OK) {
        if (R.data_error && one_pass_possible) { *fallback = true; return RAFT_HIP_OK; }
        c->last_error = R.chain.error_text;
        if (summary) *summary = tot;
        return R.chain.error;
    }
    // (a chunk that wrote its closing offsets before its successor wrote its first ones: the successor's are the same values)
    tot.total_windows = tot.n_bins;
    o->n_exc = R.base_exc;
    if (summary) *summary = tot;
    if (R.base_exc > o->exc_cap) {
        c->last_error = "raft_hip_run_multi: more windows at or above the encoding's limit than exc_cap (out->n_exc holds the number)";
        return RAFT_HIP_ERR_TOO_LARGE;
    }
    return RAFT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Chunked host pipeline: H2D, pass and D2H of consecutive read ranges overlap (PCIe is full duplex; the pass itself is
// two orders of magnitude shorter than either transfer).
//
// A read's outputs depend on nothing but the records whose query is that read (symmetric PAF, repeat.hpp:48-58), so the
// job is cut into chunks of consecutive reads.  hifiasm's PAF is a handful of runs sorted by query id (bucket.hpp), so
// a chunk's records are one contiguous piece per run: the pieces are found on the host by binary search in the
// page-locked qid column and uploaded back to back.  The cut is a guess from samples -- what makes it safe is the
// device: the pieces tile [0, n_rec) by construction, and inspect_kernel rejects any record whose (rebased) query id
// falls outside its chunk's reads; on any such report the whole job is redone in one piece.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct ChunkResult {
    long long n_bins = 0, n_rep = 0, n_frag = 0, n_exc = 0, n_cuts = 0, n_iv = 0;
    long long tot_cov = 0, tot_rep = 0, tot_len = 0;
    int path = 0;
    int graded = 0;          // RAFT_HIP_SUM_GRADED_RANGES of the chunk's pass
};

struct PipeShared : TicketChain {                   // the chain of one context's chunks (positions within the context's job)
    std::mutex down_mu;
    int uploaded = 0;                               // chunks whose H2D has been enqueued (ticket of the upload stream)
    int published = 0;                              // chunks whose sizes are known (bases of the next chunk)
    long long base_bins = 0, base_rep = 0, base_frag = 0;
};

// The chunks of one context's job are derived in order by T workers that stay for the whole job -- worker t takes the t-th slice
// of every piece -- into a ring of page-locked staging slots; a lane uploads chunk k when all workers are through with it and
// hands its slot back when the upload is done.  (The first version had every lane derive its own chunk with threads made for
// the purpose: four derivations at a time, each behind its lane's previous chunk, left the link idle a third of the time.)
struct DeriveRing {
    static constexpr int R = 3;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> done;            // workers through with chunk k
    std::vector<char> released, bad;
    bool stop = false;
    int T = 1;
    size_t slot_bytes = 0, off_bytes = 0;
    char *base = nullptr;
    long long *off_of(int kk) const { return reinterpret_cast<long long *>(base + (size_t)(kk % R) * slot_bytes); }
    uint32_t *win_of(int kk) const { return reinterpret_cast<uint32_t *>(base + (size_t)(kk % R) * slot_bytes + off_bytes); }
    bool wait_for_slot(int kk)        // a worker, before chunk kk; false: the ring was stopped
    {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return stop || kk < R || released[(size_t)(kk - R)]; });
        return !stop;
    }
    void slice_done(int kk, bool good)
    {
        std::lock_guard<std::mutex> g(mu);
        if (!good) bad[(size_t)kk] = 1;
        if (++done[(size_t)kk] == T) cv.notify_all();
    }
    bool wait_for_chunk(int kk, bool *bad_chunk)      // a lane, before the upload of chunk kk; false: the ring was stopped
    {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return stop || done[(size_t)kk] == T; });
        *bad_chunk = bad[(size_t)kk] != 0;
        return !stop;
    }
    void release(int kk) { std::lock_guard<std::mutex> g(mu); released[(size_t)kk] = 1; cv.notify_all(); }
    void halt() { std::lock_guard<std::mutex> g(mu); stop = true; cv.notify_all(); }
};

// Everything one context (one device) does in a multi-context job: its chunks, where its outputs start in the
// caller's arrays (JobPlace: windows are known in advance; repeats, fragments and exceptions are not, so every job after
// the first starts at an upper bound and is moved down when all are done), and the chain that hands each chunk the sizes
// of the chunks before it.
struct DeviceJob : JobPlace {
    raft_hip_ctx *c = nullptr;
    PipeShared sh;
    DeriveRing *ring = nullptr;                      // (derived input)
    long long n_bins = 0, n_rep = 0, n_frag = 0;     // totals of the job (valid after the run)
};

// What the phases of a chunked job share.
struct PipelinePlan {
    raft_hip_ctx *const *ctxs = nullptr;
    int32_t n_ctx = 0;
    raft_hip_ctx *c = nullptr;                       // the first context: its parameters are the job's
    HostInput in;
    int32_t n_chunks = 0;                            // as asked for (0: the engine chooses)
    raft_hip_host_outputs *o = nullptr;
    raft_hip_summary *summary = nullptr;
    bool d4 = false;                                 // four-bit steps (pack.hpp): chunks must begin on multiples of 4 windows
    int cov_width = 1;                               // bytes per window of the coverage's transfer encoding (or the delta4 code)
    int n_seg = -1;                                  // sorted runs of the record stream
    long long seg[kMaxSeg + 1] = {};
    bool done = false;                               // the routed path took the job: `result` is the call's
    int result = RAFT_HIP_OK;
    bool derive = false;                             // plain columns: offsets and window records are derived chunk by chunk
    int derive_threads = 1;
    std::vector<ChunkPlan> plan;
    int n_ch = 0, n_job = 0;
    PlaceCaps caps;
    std::vector<DeviceJob> jobs;
    std::vector<std::unique_ptr<DeriveRing>> rings;
    std::vector<ChunkResult> res;
    std::vector<std::unique_ptr<SetupGuard>> lent;   // the other contexts under the first one's parameters: their own come back with the call
    // Exceptions (windows at or above the encoding's limit) have no useful bound per device -- one device may hold all the
    // repeat-rich reads -- so every chunk takes its room from ONE cursor over the caller's list; chunks of different
    // devices interleave there and are put into read order when all are done.  A chunk that no longer fits still counts:
    // the call then returns RAFT_HIP_ERR_TOO_LARGE with the total in out->n_exc, and one retry suffices.
    std::atomic<long long> exc_cursor{0};
    std::vector<long long> exc_at;
    std::atomic<bool> redo{false};                   // a chunk reported a data error: the job is redone in one piece
    int err = RAFT_HIP_OK;                           // first failure of a job's chain
    bool trace = false;                              // RAFT_PIPE_TRACE: host-clock stamps per chunk and stage on stderr
    std::chrono::steady_clock::time_point t_origin;
    bool grouped() const { return in.rec_offset != nullptr; }   // (window records are a grouped form too)
    void stamp(int k, const char *what) const
    {
        if (trace) fprintf(stderr, "PIPE chunk %2d %-12s %8.3f ms\n", k, what,
                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_origin).count());
    }
};

int one_piece(PipelinePlan &P) { return run_monolithic_to_host(P.c, P.in, P.o, P.summary); }

int check_arguments(PipelinePlan &P)
{
    raft_hip_ctx *const *ctxs = P.ctxs;
    const HostInput &in = P.in;
    raft_hip_host_outputs *o = P.o;
    if (!ctxs || P.n_ctx < 1 || !ctxs[0] || !o) return RAFT_HIP_ERR_PARAM;
    raft_hip_ctx *c = P.c = ctxs[0];
    const bool grouped = P.grouped();
    if (in.win && (!grouped || c->prm.reso > 32767)) return RAFT_HIP_ERR_PARAM;
    if (grouped && (in.n_runs < 1 || in.n_runs > kMaxRuns || c->prm.symmetric_mode != 1)) return RAFT_HIP_ERR_PARAM;
    for (int d = 1; d < P.n_ctx; ++d) {
        if (!ctxs[d]) return RAFT_HIP_ERR_PARAM;
        for (int e = 0; e < d; ++e) if (ctxs[e] == ctxs[d]) return RAFT_HIP_ERR_PARAM;   // (two contexts may share a device)
    }
    if (in.n_reads < 0 || in.n_rec < 0 || P.n_chunks < 0) return RAFT_HIP_ERR_PARAM;
    if (in.n_reads > 0 && !in.read_len) return RAFT_HIP_ERR_PARAM;
    if (in.n_rec > 0 && ((!in.qid && !grouped) || ((!in.qs || !in.qe) && !in.win))) return RAFT_HIP_ERR_PARAM;
    if (!o->cov_offset || !o->rep_offset || !o->frag_offset) return RAFT_HIP_ERR_PARAM;
    o->n_exc = 0;
    // (more runs than the chunk plan keeps pieces for -- a PAF concatenated from many files: one piece, merged on the device)
    if (grouped && in.n_runs > kMaxSeg) return in.n_rec < (1LL << 29) ? kOnePiece : RAFT_HIP_ERR_TOO_LARGE;
    if (o->cov_width != 0 && o->cov_width != 1 && o->cov_width != 2 && o->cov_width != kCovDelta4) return RAFT_HIP_ERR_PARAM;
    P.d4 = o->cov_width == kCovDelta4;
    if (P.d4 && (!o->cov_anchor || !o->cov8)) return RAFT_HIP_ERR_PARAM;
    P.cov_width = transfer_width(o->cov_width);
    return RAFT_HIP_OK;
}

// one piece, the host-routed path (P.done) or the chunked pipeline (P.n_seg >= 1)
int choose_route(PipelinePlan &P)
{
    const HostInput &in = P.in;
    raft_hip_ctx *c = P.c;
    const bool grouped = P.grouped();
    // chunking needs: the symmetric flag asserted, enough work to split, a record stream of at most kMaxSeg sorted runs
    const bool big = big_enough(in.n_rec, in.n_reads, P.n_chunks);
    const bool eligible = c->prm.symmetric_mode == 1 && big && !c->force_bucket;
    long long (&seg)[kMaxSeg + 1] = P.seg;
    P.n_seg = -1;
    if (eligible && grouped) {                       // the runs are what the offsets say (looked at where the plan uses them)
        P.n_seg = in.n_runs;
        for (int g = 0; g < in.n_runs; ++g) seg[g] = in.off_at(g, 0);
        seg[in.n_runs] = in.n_rec;
        for (int g = 0; g < in.n_runs; ++g)
            if (seg[g] < 0 || seg[g] > seg[g + 1] || in.off_at(g, in.n_reads) != seg[g + 1]) P.n_seg = -1;   // (the one-piece pass reports it)
        if (seg[0] != 0) P.n_seg = -1;
    } else if (eligible) P.n_seg = guess_segments(in.qid, in.n_rec, seg);
    if (P.n_seg >= 1) return RAFT_HIP_OK;
    // not a handful of sorted runs (or not symmetric): several contexts, an explicit chunk count or more records than one
    // pass takes send the job through the host-routed path; anything else is one piece on the first context
    // (the routed path cuts its chunks where the host's buckets end: no multiples of 1024 windows -- delta4 stays in one piece)
    const bool route = !grouped && !P.d4 && in.n_rec > 0 && in.n_reads > 0 && !c->force_bucket &&
                       ((big && (P.n_ctx > 1 || P.n_chunks > 1)) || in.n_rec >= (1LL << 29));
    if (route) {
        bool fallback = false;
        P.result = run_routed(P.ctxs, P.n_ctx, in, P.n_chunks, P.o, P.summary, &fallback);
        P.done = !fallback;
        if (P.done) return RAFT_HIP_OK;
    }
    return kOnePiece;
}

// plain columns of a symmetric stream in a few sorted runs: the lanes derive offsets and window records chunk by chunk
int decide_derive(PipelinePlan &P)
{
    const HostInput &in = P.in;
    raft_hip_ctx *c = P.c;
    P.derive = in.form() == HostInput::kColumns && c->prm.symmetric_mode == 1 && c->prm.reso <= 32767 && P.n_seg <= kWinMaxRuns &&
               getenv("RAFT_NO_DERIVE") == nullptr;
    if (!P.derive) return RAFT_HIP_OK;
    const long long max_len = 65535LL * c->prm.reso;      // (reads of more windows than a record's 16 bits hold keep their coordinate columns)
    std::atomic<bool> fits{true};
    const int Tl = (int)std::min<long long>(16, std::max<long long>(1, in.n_reads / (1 << 18)));
    host_parallel(Tl, [&](int t) {
        const long long a = (long long)in.n_reads * t / Tl, b = (long long)in.n_reads * (t + 1) / Tl;
        bool f = true;
        for (long long i = a; i < b; ++i) f = f && in.read_len[i] <= max_len;
        if (!f) fits.store(false);
    });
    P.derive = fits.load();
    if (P.derive) {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        P.derive_threads = (int)std::max(1u, std::min(16u, hw / 4u));
        if (const char *e = getenv("RAFT_DERIVE_THREADS")) P.derive_threads = std::max(1, atoi(e));
    }
    return RAFT_HIP_OK;
}

int plan_chunks(PipelinePlan &P)
{
    const HostInput &in = P.in;
    const int want = P.n_chunks > 0 ? std::min(P.n_chunks, in.n_reads) : (int)default_chunks(in.n_rec, in.n_reads, P.n_ctx);
    // (derived input: the first chunk's derivation and the last chunk's pass and download are not hidden behind anything --
    // those two chunks are half the others' size)
    const bool ramp = P.derive && P.n_chunks == 0 && want >= 6;
    P.plan = raft::plan_chunks(in, P.seg, P.n_seg, want, ramp, P.d4, P.c->prm.reso);   // (empty: a negative read length, reported by the one-piece pass)
    P.n_ch = (int)P.plan.size();
    return P.n_ch < 2 ? kOnePiece : RAFT_HIP_OK;
}

// contexts: consecutive chunks each, and where their outputs start in the caller's arrays
int place_jobs(PipelinePlan &P)
{
    raft_hip_ctx *c = P.c;
    P.n_job = std::min(P.n_ctx, P.n_ch);
    const std::vector<JobPlace> at = raft::place_jobs(P.plan, P.n_job, P.in.read_len, c->minbins, c->prm.interval_length, WindowDiv(c->prm.reso), &P.caps);
    if (at.empty()) return kOnePiece;                // (a negative read length: reported as RAFT_HIP_ERR_PARAM with its index by the one-piece pass)
    P.jobs = std::vector<DeviceJob>((size_t)P.n_job);
    for (int d = 0; d < P.n_job; ++d) {
        static_cast<JobPlace &>(P.jobs[(size_t)d]) = at[(size_t)d];
        P.jobs[(size_t)d].c = P.ctxs[d];
        P.jobs[(size_t)d].sh.also_stop = &P.redo;
    }
    return RAFT_HIP_OK;
}

// parameters of the first context for all (until the call returns), the lanes; then the caller's capacities against what the placement needs
int prepare_contexts(PipelinePlan &P)
{
    raft_hip_ctx *c = P.c;
    raft_hip_host_outputs *o = P.o;
    for (int d = 0; d < P.n_job; ++d) {
        raft_hip_ctx *jc = P.jobs[(size_t)d].c;
        if (d > 0) {
            // (as the routed path does; a pass of its own that the context holds is dropped by drain_and_collect, once lanes have run)
            P.lent.push_back(std::make_unique<SetupGuard>(jc, &c->prm, jc->out_width, true));
            jc->tile_q = c->tile_q;
        }
        const int rc = prepare_lanes(jc);
        if (rc != RAFT_HIP_OK) return rc;
    }
    if (P.n_job == 1) {                              // one context: the caller's capacities are the only limits
        P.jobs[0].rep_room = o->rep_cap; P.jobs[0].frag_room = o->frag_cap;
    } else if (P.caps.rep > o->rep_cap || P.caps.frag > o->frag_cap || (o->cov8 && P.caps.bins > o->cov8_cap) ||
               (P.d4 && (P.caps.bins + kD4Block - 1) / kD4Block > o->anchor_cap)) {
        c->last_error = "raft_hip_run_multi: cov8_cap / rep_cap / frag_cap below the bounds stated in raft_hip.h";
        return RAFT_HIP_ERR_TOO_LARGE;
    }
    return RAFT_HIP_OK;
}

// derived input: every job's ring of page-locked slots, each as large as the job's largest chunk needs
int make_rings(PipelinePlan &P)
{
    P.rings.resize((size_t)P.n_job);
    if (!P.derive) return RAFT_HIP_OK;
    for (int d = 0; d < P.n_job; ++d) {
        DeviceJob &J = P.jobs[(size_t)d];
        auto ring = std::make_unique<DeriveRing>();
        size_t off_b = 0, win_b = 0;
        for (int kk = 0; kk < J.n_chunks; ++kk) {
            const ChunkPlan &cp = P.plan[(size_t)(J.first_chunk + kk)];
            off_b = std::max(off_b, (size_t)P.n_seg * ((size_t)(cp.r1 - cp.r0) + 1) * 8);
            win_b = std::max(win_b, (size_t)std::max<long long>(cp.n_rec, 1) * 4);
        }
        ring->off_bytes = (off_b + 255) & ~(size_t)255;
        ring->slot_bytes = (ring->off_bytes + win_b + 255) & ~(size_t)255;
        const size_t need = ring->slot_bytes * DeriveRing::R;
        const int rc = ensure_stage(J.c, need, need / 8);
        if (rc != RAFT_HIP_OK) return rc;
        ring->base = reinterpret_cast<char *>(J.c->h_stage);
        ring->T = P.derive_threads;
        ring->done.assign((size_t)J.n_chunks, 0); ring->released.assign((size_t)J.n_chunks, 0); ring->bad.assign((size_t)J.n_chunks, 0);
        J.ring = ring.get();
        P.rings[(size_t)d] = std::move(ring);
    }
    (void)hipSetDevice(P.c->device);
    return RAFT_HIP_OK;
}

// worker t of job J's ring: slice t of every piece of every chunk, in chunk order
void derive_worker(const PipelinePlan &P, DeviceJob &J, int t)
{
    DeriveRing &R = *J.ring;
    const HostInput &in = P.in;
    const WindowDiv div(P.c->prm.reso);
    for (int kk = 0; kk < J.n_chunks; ++kk) {
        if (!R.wait_for_slot(kk)) return;
        const ChunkPlan &cp = P.plan[(size_t)(J.first_chunk + kk)];
        const int32_t nr = cp.r1 - cp.r0;
        long long at = 0;
        bool good = true;
        for (int g = 0; g < P.n_seg; ++g) {
            good = derive_slice(t, R.T, in.qid, in.qs, in.qe, cp.piece[g].lo, cp.piece[g].hi, cp.r0, cp.r1, div, at, R.off_of(kk) + (long long)g * (nr + 1),
                                R.win_of(kk) + at) && good;
            at += cp.piece[g].hi - cp.piece[g].lo;
        }
        R.slice_done(kk, good);
    }
}

enum class Step { kGoOn, kStop, kRedo };            // a stage's answer: the next stage; the lane ends; the job is redone in one piece

// One lane of a job: every kLanes-th chunk of the job's chain through the stages below, on the lane's own sub-context.
struct Lane {
    PipelinePlan &P;
    DeviceJob &J;
    const int li;
    raft_hip_ctx *const jc, *const l;
    PipeShared &sh;
    // the chunk in hand
    int kk = 0, k = 0;                               // position in the job's chain; global chunk index
    const ChunkPlan *cp = nullptr;
    ChunkResult *cr = nullptr;
    int32_t nr = 0;
    long long *st_off = nullptr;                     // derived input: the chunk's slot of the ring
    uint32_t *st_win = nullptr;
    long long b_bins = 0, b_rep = 0, b_frag = 0, b_exc = 0;
    bool exc_fits = false;

    Lane(PipelinePlan &P_, DeviceJob &J_, int li_) : P(P_), J(J_), li(li_), jc(J_.c), l(J_.c->lanes[(size_t)li_]), sh(J_.sh) {}
    Step fail(int code, const std::string &text) { sh.fail(code, text); return Step::kStop; }
    Step hip(hipError_t e, const char *what) { return e == hipSuccess ? Step::kGoOn : fail(fail_hip(l, e, what), l->last_error); }
    Step ensure_inputs();
    Step await_derived();
    Step upload();
    Step run_pass_on_chunk();
    Step take_bases();
    Step download();
    Step copy_down(int i, void *dst, const void *src, size_t bytes);
    void run();
};

Step Lane::ensure_inputs()
{
    const HostInput &in = P.in;
    const bool offsets = P.grouped() || P.derive;
    hipError_t e = l->in_len.ensure((size_t)std::max(nr, 1) * 4);
    const int col_end = (in.win || P.derive) ? 2 : 3;          // (window records: one column)
    for (int col = offsets ? 1 : 0; col < col_end && e == hipSuccess; ++col) e = l->in_col[col].ensure((size_t)std::max<long long>(cp->n_rec, 1) * 4);
    if (offsets && e == hipSuccess) e = l->in_off.ensure((size_t)P.n_seg * ((size_t)nr + 1) * 8);
    return hip(e, "a lane's input buffers");
}

// the chunk's offsets and window records: derived by the job's workers while earlier chunks travel
Step Lane::await_derived()
{
    if (!P.derive) return Step::kGoOn;
    bool bad_chunk = false;
    const bool running = J.ring->wait_for_chunk(kk, &bad_chunk);
    P.stamp(k, "derived");
    if (!running) return Step::kStop;
    if (bad_chunk) return Step::kRedo;               // (the one-piece pass over the columns reports or handles it)
    st_off = J.ring->off_of(kk); st_win = J.ring->win_of(kk);
    return Step::kGoOn;
}

// in chunk order on the one upload stream (the link is the bottleneck: first come, first served)
Step Lane::upload()
{
    const HostInput &in = P.in;
    const bool grouped = P.grouped(), derive = P.derive;
    const int n_seg = P.n_seg;
    hipStream_t up = jc->up_stream;
    if (!sh.await(sh.uploaded, kk).owns_lock()) return Step::kStop;
    hipError_t e = hipMemcpyAsync(l->in_len.p, in.read_len + cp->r0, (size_t)nr * 4, hipMemcpyHostToDevice, up);
    if (derive) {
        if (e == hipSuccess) e = hipMemcpyAsync(l->in_off.p, st_off, (size_t)n_seg * ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, up);
        if (e == hipSuccess && cp->n_rec > 0) e = hipMemcpyAsync(l->in_col[1].p, st_win, (size_t)cp->n_rec * 4, hipMemcpyHostToDevice, up);
    }
    const int32_t *src[3] = {in.qid, in.win ? reinterpret_cast<const int32_t *>(in.win) : in.qs, in.qe};
    const int col_end = (in.win || derive) ? 2 : 3;
    // (grouped: a slice of every run's offsets instead of the query column -- 8 bytes per read and run, not 4 per record)
    for (int g = 0; grouped && !derive && g < n_seg && e == hipSuccess; ++g)
        e = hipMemcpyAsync(l->in_off.as<long long>() + (long long)g * (nr + 1), in.rec_offset + (long long)g * ((long long)in.n_reads + 1) + cp->r0,
                           (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, up);
    for (int col = grouped ? 1 : 0; !derive && col < col_end && e == hipSuccess; ++col) {
        long long at = 0;
        for (int g = 0; g < n_seg && e == hipSuccess; ++g) {
            const long long n = cp->piece[g].hi - cp->piece[g].lo;
            if (n > 0) e = hipMemcpyAsync(l->in_col[col].as<int32_t>() + at, src[col] + cp->piece[g].lo, (size_t)n * 4, hipMemcpyHostToDevice, up);
            at += n;
        }
    }
    if (e == hipSuccess) e = hipEventRecord(jc->lane_up_ev[(size_t)li], up);
    P.stamp(k, "h2d queued");
    {   // the ticket goes on before the copies' error is acted on: a failing upload must not strand the next lane
        std::lock_guard<std::mutex> g(sh.mu);
        sh.hand_on(sh.uploaded, kk);
    }
    if (e != hipSuccess) return hip(e, "a chunk's upload");
    // The lane's thread waits for the upload itself.  A wait-event parked in the lane's stream would sit in a
    // hardware queue that other lanes' streams share, and hold THEIR kernels until this chunk's upload is done
    // (measured: chunks whose pass was queued at 12 ms ran at 24 ms).
    e = hipEventSynchronize(jc->lane_up_ev[(size_t)li]);
    if (e != hipSuccess) return hip(e, "hipEventSynchronize(upload)");
    P.stamp(k, "h2d done");
    if (derive) J.ring->release(kk);
    if (cp->n_rec > 0 && cp->r0 != 0 && !grouped && !derive) launch_rebase_ids(l->stream, l->in_col[0].as<int32_t>(), cp->n_rec, cp->r0);
    return Step::kGoOn;
}

Step Lane::run_pass_on_chunk()
{
    const HostInput &in = P.in;
    const int n_seg = P.n_seg;
    raft_hip_summary s{};
    l->out_width = P.cov_width;            // the pass writes the encoding that travels
    l->d4_shift = P.d4 ? (int)(cp->win_lo & (kD4Block - 1)) : 0;
    int rc;
    if (P.derive) {
        // (the staged offsets count from the chunk's own first record: nothing to rebase)
        const long long hint = count_windows(in.read_len + cp->r0, nr, WindowDiv(P.c->prm.reso));
        rc = run_grouped(l, nr, l->in_len.as<int32_t>(), cp->n_rec, n_seg, l->in_off.as<int64_t>(), nullptr, nullptr, nullptr, nullptr, hint,
                         cp->n_rec > 0 ? l->in_col[1].as<uint32_t>() : nullptr);
    } else if (P.grouped()) {
        // the chunk's pieces lie back to back on the device: run g's slice of offsets counts from the caller's
        // stream and is moved by adj[g] to where the piece went
        long long adj[kMaxSeg] = {0, 0, 0, 0}, at = 0;
        for (int g = 0; g < n_seg; ++g) { adj[g] = at - cp->piece[g].lo; at += cp->piece[g].hi - cp->piece[g].lo; }
        const long long hint = count_windows(in.read_len + cp->r0, nr, WindowDiv(P.c->prm.reso));
        if (in.win) rc = run_grouped(l, nr, l->in_len.as<int32_t>(), cp->n_rec, n_seg, l->in_off.as<int64_t>(), adj, nullptr, nullptr, nullptr, hint,
                                     l->in_col[1].as<uint32_t>());
        else rc = run_grouped(l, nr, l->in_len.as<int32_t>(), cp->n_rec, n_seg, l->in_off.as<int64_t>(), adj, nullptr,
                              l->in_col[1].as<int32_t>(), l->in_col[2].as<int32_t>(), hint);
    } else
        rc = raft_hip_run_device(l, nr, l->in_len.as<int32_t>(), cp->n_rec, l->in_col[0].as<int32_t>(),
                                 l->in_col[1].as<int32_t>(), l->in_col[2].as<int32_t>(), nullptr, nullptr, nullptr);
    P.stamp(k, "pass queued");
    if (rc == RAFT_HIP_OK) rc = raft_hip_finish(l, &s);
    P.stamp(k, "pass done");
    if (is_data_error(rc)) return Step::kRedo;
    if (rc != RAFT_HIP_OK) return fail(rc, l->last_error);
    rc = pack_coverage(l, P.cov_width);
    if (rc == RAFT_HIP_OK) rc = sort_exceptions(l);          // (ascending by window, like raft_hip_fetch_packed)
    if (rc != RAFT_HIP_OK) return fail(rc, l->last_error);
    P.stamp(k, "packed");
    cr->n_bins = s.n_bins; cr->n_rep = s.n_repeats; cr->n_frag = s.n_fragments; cr->n_exc = l->n_exc; cr->n_cuts = s.n_cuts;
    cr->n_iv = s.n_intervals; cr->tot_cov = s.total_coverage; cr->tot_rep = s.total_repeat_length; cr->tot_len = s.total_read_length;
    cr->path = s.interval_path; cr->graded = s.flags & RAFT_HIP_SUM_GRADED_RANGES;
    return Step::kGoOn;
}

// where this chunk's outputs go: after those of the job's earlier chunks
Step Lane::take_bases()
{
    raft_hip_host_outputs *o = P.o;
    auto turn = sh.await(sh.published, kk);
    if (!turn.owns_lock()) return Step::kStop;
    b_bins = J.bins0 + sh.base_bins; b_rep = J.rep0 + sh.base_rep; b_frag = J.frag0 + sh.base_frag;
    b_exc = P.exc_cursor.fetch_add(cr->n_exc);
    P.exc_at[(size_t)k] = b_exc;
    exc_fits = b_exc + cr->n_exc <= o->exc_cap;
    sh.base_bins += cr->n_bins; sh.base_rep += cr->n_rep; sh.base_frag += cr->n_frag;
    if (sh.base_rep > J.rep_room || sh.base_frag > J.frag_room || (o->cov8 && J.bins0 + sh.base_bins > o->cov8_cap) ||
        (P.d4 && (J.bins0 + sh.base_bins + kD4Block - 1) / kD4Block > o->anchor_cap)) {
        if (sh.error == RAFT_HIP_OK) { sh.error = RAFT_HIP_ERR_TOO_LARGE; sh.error_text = "host output capacity (coverage / repeats / fragments)"; }
    }
    sh.hand_on(sh.published, kk);
    return sh.error != RAFT_HIP_OK ? Step::kStop : Step::kGoOn;
}

// one copy of a chunk's download (down_mu held)
Step Lane::copy_down(int i, void *dst, const void *src, size_t bytes)
{
    if (!dst || !bytes) return Step::kGoOn;
    // (trace: a copy call that holds its caller.  In a process's first passes one or two of them take ~7 ms of
    // the caller's CPU time each, whatever their size: the runtime picks another SDMA engine when the stream's
    // last one is busy, and an engine's first use sets its queue up -- hsa_amd_memory_async_copy_on_engine ->
    // a KFD SVM ioctl, profiles/r06_sdma_first_use.txt.  A long-lived context stops seeing them.)
    timespec c0{}, c1{};
    const auto w0 = std::chrono::steady_clock::now();
    if (P.trace) clock_gettime(CLOCK_THREAD_CPUTIME_ID, &c0);
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, jc->down_stream);
    if (e != hipSuccess) return hip(e, "a chunk's download");
    if (P.trace) {
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &c1);
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        if (wall > 0.5)
            fprintf(stderr, "PIPE chunk %2d d2h copy %d of %zu bytes held its caller %.3f ms (thread cpu %.3f ms)\n", k, i, bytes, wall,
                    (c1.tv_sec - c0.tv_sec) * 1e3 + (c1.tv_nsec - c0.tv_nsec) * 1e-6);
        P.stamp(k, "d2h copy");
    }
    return Step::kGoOn;
}

Step Lane::download()
{
    raft_hip_host_outputs *o = P.o;
    const bool d4 = P.d4;
    const int cov_width = P.cov_width;
    hipStream_t st = l->stream;
    const long long n1 = (long long)nr + ((k == P.n_ch - 1) ? 1 : 0);   // the closing entry belongs to the last chunk
    auto add_base = [&](DevBuf &b, long long n, long long base) {
        if (base != 0 && n > 0) launch_add_base(st, b.as<long long>(), n, base);
    };
    // offsets count from the job's first entry (rep / frag of later jobs are moved down afterwards)
    add_base(l->cov_off, n1, b_bins); add_base(l->rep_off, n1, b_rep - J.rep0); add_base(l->frag_off, n1, b_frag - J.frag0);
    add_base(l->exc_idx, cr->n_exc, b_bins);
    const int d4_sh = l->d4_shift, d4_j0 = d4_sh ? 1 : 0;
    if (d4 && b_bins != cp->win_lo) return fail(RAFT_HIP_ERR_DEVICE, "delta4: a chunk's windows do not begin where the plan put them");
    struct { void *dst; const void *src; size_t bytes; } job[] = {
        {o->cov8 ? o->cov8 + (d4 ? b_bins / 2 : b_bins * cov_width) : nullptr, l->cov8.p,
         d4 ? ((size_t)cr->n_bins + 1) / 2 : (size_t)cr->n_bins * (size_t)cov_width},
        // (anchors: the block the chunk begins in belongs to the chunk before unless it begins with it)
        {d4 ? o->cov_anchor + (b_bins - d4_sh) / kD4Block + d4_j0 : nullptr, l->cov_anchor.as<int32_t>() + d4_j0,
         d4 ? (size_t)(((long long)d4_sh + cr->n_bins + kD4Block - 1) / kD4Block - d4_j0) * 4 : 0},
        {o->cov_offset + cp->r0, l->cov_off.p, (size_t)n1 * 8},
        {(o->exc_index && exc_fits) ? o->exc_index + b_exc : nullptr, l->exc_idx.p, (size_t)cr->n_exc * 8},
        {(o->exc_value && exc_fits) ? o->exc_value + b_exc : nullptr, l->exc_val.p, (size_t)cr->n_exc * 4},
        {o->rep_offset + cp->r0, l->rep_off.p, (size_t)n1 * 8},
        {o->rep_s ? o->rep_s + b_rep : nullptr, l->rep_s.p, (size_t)cr->n_rep * 4},
        {o->rep_e ? o->rep_e + b_rep : nullptr, l->rep_e.p, (size_t)cr->n_rep * 4},
        {o->frag_offset + cp->r0, l->frag_off.p, (size_t)n1 * 8},
        {o->frag_begin ? o->frag_begin + b_frag : nullptr, l->frag_begin.p, (size_t)cr->n_frag * 4},
        {o->frag_end ? o->frag_end + b_frag : nullptr, l->frag_end.p, (size_t)cr->n_frag * 4}};
    // the download stream takes over once the lane's last kernel is done; the lane waits for its own copies only
    hipEvent_t ev = jc->lane_down_ev[(size_t)li];
    P.stamp(k, "bases known");
    Step step = hip(hipEventRecord(ev, st), "hipEventRecord(a lane's last kernel)");
    if (step != Step::kGoOn) return step;
    {
        std::lock_guard<std::mutex> g(sh.down_mu);       // one chunk's copies stay together on the stream
        step = hip(hipStreamWaitEvent(jc->down_stream, ev, 0), "hipStreamWaitEvent(download)");
        if (step != Step::kGoOn) return step;
        P.stamp(k, "d2h wait set");
        for (auto &j : job)
            if ((step = copy_down((int)(&j - job), j.dst, j.src, j.bytes)) != Step::kGoOn) return step;
        step = hip(hipEventRecord(ev, jc->down_stream), "hipEventRecord(download)");
        if (step != Step::kGoOn) return step;
    }
    P.stamp(k, "d2h queued");
    step = hip(hipEventSynchronize(ev), "hipEventSynchronize(download)");
    if (step == Step::kGoOn) P.stamp(k, "d2h done");
    return step;
}

void Lane::run()
{
    static constexpr Step (Lane::*kStages[])() = {&Lane::ensure_inputs, &Lane::await_derived, &Lane::upload,
                                                 &Lane::run_pass_on_chunk, &Lane::take_bases, &Lane::download};
    Step step = Step::kGoOn;
    if (hipSetDevice(jc->device) != hipSuccess) step = fail(RAFT_HIP_ERR_DEVICE, "hipSetDevice");
    for (kk = li; kk < J.n_chunks && step == Step::kGoOn; kk += kLanes) {
        k = J.first_chunk + kk;
        cp = &P.plan[(size_t)k];
        cr = &P.res[(size_t)k];
        nr = cp->r1 - cp->r0;
        for (auto stage : kStages)
            if ((step = (this->*stage)()) != Step::kGoOn) break;
    }
    if (step == Step::kRedo) P.redo.store(true);
    // a lane that stops early must not leave the others waiting for its tickets, nor the workers for its slots
    const bool stopped = sh.wake();
    if (P.derive && stopped) J.ring->halt();
}

int run_lanes(PipelinePlan &P)
{
    P.res.assign((size_t)P.n_ch, ChunkResult{});
    P.exc_at.assign((size_t)P.n_ch, 0);
    P.trace = getenv("RAFT_PIPE_TRACE") != nullptr;
    P.t_origin = std::chrono::steady_clock::now();
    auto lane_main = [&P](int d, int li) { Lane(P, P.jobs[(size_t)d], li).run(); };
    std::vector<std::thread> th, workers;
    if (P.derive)
        for (int d = 0; d < P.n_job; ++d)
            for (int t = 0; t < P.derive_threads; ++t) workers.emplace_back([&P, d, t] { derive_worker(P, P.jobs[(size_t)d], t); });
    for (int d = 0; d < P.n_job; ++d)
        for (int li = 0; li < kLanes; ++li)
            if (d || li) th.emplace_back(lane_main, d, li);
    lane_main(0, 0);
    for (auto &t : th) t.join();
    if (P.derive)
        for (DeviceJob &J : P.jobs) J.ring->halt();       // (a job that ended early leaves workers waiting for slots)
    for (auto &t : workers) t.join();
    return RAFT_HIP_OK;
}

// every stream idle, the contexts hold no pass; the first error, the summary, the number of exceptions
int drain_and_collect(PipelinePlan &P)
{
    raft_hip_ctx *c = P.c;
    raft_hip_host_outputs *o = P.o;
    for (DeviceJob &J : P.jobs) {
        (void)hipSetDevice(J.c->device);
        (void)hipStreamSynchronize(J.c->up_stream);
        (void)hipStreamSynchronize(J.c->down_stream);
        for (raft_hip_ctx *l : J.c->lanes) (void)hipStreamSynchronize(l->stream);
        J.c->ran = false; J.c->finished = false;   // the contexts hold no pass: fetch / outputs_device do not apply
        J.n_bins = J.sh.base_bins; J.n_rep = J.sh.base_rep; J.n_frag = J.sh.base_frag;
        if (J.sh.error != RAFT_HIP_OK && P.err == RAFT_HIP_OK) { P.err = J.sh.error; c->last_error = J.sh.error_text; }
    }
    (void)hipSetDevice(c->device);
    if (P.redo.load()) return kOnePiece;

    raft_hip_summary s{};
    s.n_reads = P.in.n_reads; s.symmetric = 1; s.high_cov = c->high_cov; s.n_segments = P.n_seg; s.n_records = P.in.n_rec; s.error_index = -1;
    s.n_devices_used = P.n_job;
    for (const ChunkResult &cr : P.res) {
        s.n_bins += cr.n_bins; s.n_repeats += cr.n_rep; s.n_fragments += cr.n_frag; s.n_cuts += cr.n_cuts; s.n_intervals += cr.n_iv;
        s.total_coverage += cr.tot_cov; s.total_repeat_length += cr.tot_rep; s.total_read_length += cr.tot_len;
        s.interval_path |= cr.path; s.flags |= cr.graded;
    }
    s.total_windows = s.n_bins;
    if (P.summary) *P.summary = s;
    if (P.err != RAFT_HIP_OK) return P.err;
    o->n_exc = P.exc_cursor.load();
    if (o->n_exc > o->exc_cap) {
        c->last_error = "raft_hip_run_multi: more windows at or above the encoding's limit than exc_cap (out->n_exc holds the number)";
        return RAFT_HIP_ERR_TOO_LARGE;
    }
    return RAFT_HIP_OK;
}

// exceptions: chunks of different devices took their room in the order they finished; hand them out in read order
int reorder_exceptions(PipelinePlan &P)
{
    raft_hip_host_outputs *o = P.o;
    if (P.n_job < 2 || o->n_exc <= 0) return RAFT_HIP_OK;
    bool ordered = true;
    long long at = 0;
    for (int k = 0; k < P.n_ch; ++k) { ordered = ordered && P.exc_at[(size_t)k] == at; at += P.res[(size_t)k].n_exc; }
    if (ordered) return RAFT_HIP_OK;
    std::vector<int64_t> ti((size_t)o->n_exc);
    std::vector<int32_t> tv((size_t)o->n_exc);
    at = 0;
    for (int k = 0; k < P.n_ch; ++k) {
        const long long n = P.res[(size_t)k].n_exc, from = P.exc_at[(size_t)k];
        if (o->exc_index) memcpy(ti.data() + at, o->exc_index + from, (size_t)n * 8);
        if (o->exc_value) memcpy(tv.data() + at, o->exc_value + from, (size_t)n * 4);
        at += n;
    }
    if (o->exc_index) memcpy(o->exc_index, ti.data(), (size_t)o->n_exc * 8);
    if (o->exc_value) memcpy(o->exc_value, tv.data(), (size_t)o->n_exc * 4);
    return RAFT_HIP_OK;
}

// later jobs wrote repeats / fragments at their upper-bound positions: close the gaps
int close_gaps(PipelinePlan &P)
{
    raft_hip_host_outputs *o = P.o;
    long long rep_at = P.jobs[0].n_rep, frag_at = P.jobs[0].n_frag;
    for (int d = 1; d < P.n_job; ++d) {
        DeviceJob &J = P.jobs[(size_t)d];
        const int32_t ra = P.plan[(size_t)J.first_chunk].r0, rb = P.plan[(size_t)(J.first_chunk + J.n_chunks - 1)].r1;
        auto move32 = [](int32_t *a, long long to, long long from, long long n) { if (a && n && to != from) memmove(a + to, a + from, (size_t)n * 4); };
        move32(o->rep_s, rep_at, J.rep0, J.n_rep); move32(o->rep_e, rep_at, J.rep0, J.n_rep);
        move32(o->frag_begin, frag_at, J.frag0, J.n_frag); move32(o->frag_end, frag_at, J.frag0, J.n_frag);
        const int32_t r_hi = rb + ((d == P.n_job - 1) ? 1 : 0);
        for (int32_t r = ra; r < r_hi; ++r) { o->rep_offset[r] += rep_at; o->frag_offset[r] += frag_at; }
        rep_at += J.n_rep; frag_at += J.n_frag;
    }
    return RAFT_HIP_OK;
}

} // namespace

static int run_multi_impl(raft_hip_ctx *const *ctxs, int32_t n_ctx, const HostInput &in, int32_t n_chunks, raft_hip_host_outputs *o,
                          raft_hip_summary *summary)
{
    PipelinePlan P;
    P.ctxs = ctxs; P.n_ctx = n_ctx; P.in = in; P.n_chunks = n_chunks; P.o = o; P.summary = summary;
    PHASE(check_arguments(P));
    PHASE(choose_route(P));
    if (P.done) return P.result;
    PHASE(decide_derive(P));
    PHASE(plan_chunks(P));
    PHASE(place_jobs(P));
    PHASE(prepare_contexts(P));
    PHASE(make_rings(P));
    PHASE(run_lanes(P));
    PHASE(drain_and_collect(P));
    PHASE(reorder_exceptions(P));
    PHASE(close_gaps(P));
    return RAFT_HIP_OK;
}

// What the first job of a fresh process pays once -- the engine's code object going to the device at the first launch, the
// four lanes (sub-contexts with their streams, events and page-locked blocks), the small per-context buffers -- is 70-80 ms
// on the MI355X box: five times the work of a 4.4e7-record job.  The CLI calls this beside the tokenising of its inputs.
int raft_hip_warm_up(raft_hip_ctx *c)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    int rc = prepare_lanes(c);
    if (rc != RAFT_HIP_OK) return rc;
    {   // the copy engines behind the pipeline's two copy streams come up at their first large copy (measured: the first
        // 40 MB download of a process sat 10 ms in hipMemcpyAsync)
        HIP_TRY(c, hipSetDevice(c->device));
        void *h = nullptr, *d = nullptr;
        const size_t n = 4u << 20;
        if (hipHostMalloc(&h, n, hipHostMallocDefault) == hipSuccess && hipMalloc(&d, n) == hipSuccess) {
            (void)hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->up_stream);
            (void)hipStreamSynchronize(c->up_stream);
            (void)hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->down_stream);
            (void)hipStreamSynchronize(c->down_stream);
        }
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        (void)hipGetLastError();
    }
    const int32_t len[2] = {400, 300}, qs[2] = {0, 10}, qe[2] = {120, 200};
    const int64_t off[3] = {0, 1, 2};
    std::vector<raft_hip_ctx *> all(c->lanes);
    all.push_back(c);
    for (raft_hip_ctx *l : all) {
        {
            const raft_hip_params p1{50, 30, 1.5, 10000, 10000, 20000, 500, 1000, 1};   // (the reference's defaults: the two reads stay whole)
            SetupGuard setup(l, &p1, 1);
            for (int w = 1; w <= 2 && rc == RAFT_HIP_OK; ++w) {           // (both widths of the transfer encoding: their own kernels)
                l->out_width = w;
                rc = raft_hip_run_host_grouped(l, 2, len, 2, 1, off, qs, qe, -1);
                raft_hip_summary s{};
                if (rc == RAFT_HIP_OK) rc = raft_hip_finish(l, &s);
            }
        }
        if (rc != RAFT_HIP_OK) { c->last_error = l->last_error; break; }
    }
    return rc;
}

// The device buffers of a job, allocated ahead of it: ~35 allocations per lane (5 ms), the staging of a chunk's columns
// (hundreds of MB: 2 ms each) -- inside the first job's clock unless somebody knows its shape earlier.  The CLI does, after
// loading the reads: their lengths, and the record count to within a few per cent from the size of the overlaps file.  A
// pass over the expected chunk's reads WITHOUT records sizes everything that follows the reads; the record-sized buffers
// are sized directly.  Buffers only grow, so an estimate that falls short costs what it would have cost anyway.
int raft_hip_reserve(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec_estimate, int32_t n_ctx, int32_t cov_width)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !read_len) || n_rec_estimate < 0 || n_ctx < 1) return RAFT_HIP_ERR_PARAM;
    if (n_reads == 0) return RAFT_HIP_OK;
    const bool chunked = big_enough(n_rec_estimate, n_reads, 0);
    const long long chunks = chunked ? std::max<long long>(1, default_chunks(n_rec_estimate, n_reads, n_ctx)) : 1;
    const int32_t nr = (int32_t)std::min<long long>(n_reads, n_reads / chunks + n_reads / chunks / 4 + 64);
    const long long nrec = n_rec_estimate / chunks + n_rec_estimate / chunks / 4 + 1024;
    int rc = RAFT_HIP_OK;
    std::vector<raft_hip_ctx *> who;
    if (chunked) {
        rc = prepare_lanes(c);
        if (rc != RAFT_HIP_OK) return rc;
        const long long per_ctx = (chunks + n_ctx - 1) / n_ctx;
        for (int li = 0; li < std::min<long long>(kLanes, per_ctx); ++li) who.push_back(c->lanes[(size_t)li]);
        // ... and the page-locked ring the lanes derive plain columns into (DeriveRing): 300 MB for a 4.4e7-record
        // job, whose page-locking was 50 of the 64 ms that job's engine call took (profiles/r06_s18_cli_s500k.txt: its two chunks
        // were through after 8 ms)
        const size_t off_b = ((size_t)kWinMaxRuns * ((size_t)nr + 1) * 8 + 255) & ~(size_t)255;
        const size_t need = ((off_b + (size_t)nrec * 4 + 255) & ~(size_t)255) * DeriveRing::R;
        if (!getenv("RAFT_NO_DERIVE")) {
            rc = ensure_stage(c, need);
            if (rc != RAFT_HIP_OK) return rc;
        }
    } else who.push_back(c);
    std::vector<int64_t> zeros((size_t)nr + 1, 0);
    for (raft_hip_ctx *l : who) {
        HIP_TRY(l, hipSetDevice(l->device));
        for (int col = 1; col < 3; ++col) HIP_TRY(l, l->in_col[col].ensure((size_t)nrec * 4));
        HIP_TRY(l, l->exp_qid.ensure((size_t)nrec * 4));
        HIP_TRY(l, l->in_off.ensure((size_t)kMaxSeg * ((size_t)nr + 1) * 8));
        {
            raft_hip_params p1 = c->prm;
            p1.symmetric_mode = 1;
            SetupGuard setup(l, &p1, transfer_width(cov_width));
            rc = raft_hip_run_host_grouped(l, nr, read_len, 0, 1, zeros.data(), nullptr, nullptr, -1);
            raft_hip_summary s{};
            if (rc == RAFT_HIP_OK) rc = raft_hip_finish(l, &s);
        }
        if (rc == RAFT_HIP_ERR_NOMEM || rc == RAFT_HIP_ERR_DEVICE) { c->last_error = l->last_error; return rc; }   // (data errors are the job's to report)
    }
    return RAFT_HIP_OK;
}

int raft_hip_run_multi(raft_hip_ctx *const *ctxs, int32_t n_ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec,
                       const int32_t *qid, const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts,
                       const int32_t *te, int32_t n_chunks, raft_hip_host_outputs *o, raft_hip_summary *summary)
{
    HostInput in;
    in.n_reads = n_reads; in.read_len = read_len; in.n_rec = n_rec;
    in.qid = qid; in.qs = qs; in.qe = qe; in.tid = tid; in.ts = ts; in.te = te;
    return run_multi_impl(ctxs, n_ctx, in, n_chunks, o, summary);
}

int raft_hip_run_multi_grouped(raft_hip_ctx *const *ctxs, int32_t n_ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec,
                               int32_t n_runs, const int64_t *rec_offset, const int32_t *qs, const int32_t *qe, int32_t n_chunks,
                               raft_hip_host_outputs *o, raft_hip_summary *summary)
{
    if (!rec_offset) return RAFT_HIP_ERR_PARAM;
    return run_multi_impl(ctxs, n_ctx, grouped_input(n_reads, read_len, n_rec, n_runs, rec_offset, qs, qe, nullptr), n_chunks, o, summary);
}

int raft_hip_run_multi_windows(raft_hip_ctx *const *ctxs, int32_t n_ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec,
                               int32_t n_runs, const int64_t *rec_offset, const uint32_t *win, int32_t n_chunks,
                               raft_hip_host_outputs *o, raft_hip_summary *summary)
{
    if (!rec_offset || (n_rec > 0 && !win)) return RAFT_HIP_ERR_PARAM;
    static const uint32_t none = 0;
    return run_multi_impl(ctxs, n_ctx, grouped_input(n_reads, read_len, n_rec, n_runs, rec_offset, nullptr, nullptr, win ? win : &none), n_chunks, o,
                          summary);
}

int raft_hip_run_pipelined(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                           const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                           int32_t n_chunks, raft_hip_host_outputs *o, raft_hip_summary *summary)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    return raft_hip_run_multi(&c, 1, n_reads, read_len, n_rec, qid, qs, qe, tid, ts, te, n_chunks, o, summary);
}


} // extern "C"
