// engine.hip -- context, launch sequence and C ABI (include/raft_hip.h) of the
// MI355X engine.  One context = one device + one stream + grow-only device
// buffers; one pass = the kernels listed in DESIGN.md §Kernels, in order.
#include "cov_decode.hpp"

#include "bucket.hpp"
#include "sort_pairs.hpp"
#include "device_scan.hpp"
#include "finalize.hpp"
#include "cov_hist.hpp"
#include "read_stats.hpp"
#include "census.hpp"
#include "pileup.hpp"
#include "pileup_wave.hpp"
#include "wave_launch.hpp"
#include "pileup_deep.hpp"

namespace {

struct ReadPrepLoader {               // per read: windows, reserved repeat slots, marker capacity
    const int32_t *len;
    int32_t reso, minbins, L;
    int32_t long_windows, piece_w;    // reads longer than long_windows are piled up in pieces of piece_w windows
    int32_t *err_flags;
    long long *err_index;
    FastDiv by_reso, by_mb1, by_L;    // reso, minbins + 1, L as divisors (three hardware divisions per read, one of them 64 bits wide,
                                      // twice per pass, were most of what the two scan kernels executed)
    int32_t *seen;                    // the lengths as this scan saw them (engine_ctx.hpp len_seen)
    __device__ void operator()(long long i, long long (&v)[3]) const
    {
        int l = len[i];
        seen[i] = l;
        if (l < 0) {
            atomicOr(err_flags, kErrLen);
            atomicMin((unsigned long long *)err_index, (unsigned long long)i);
            l = 0;
        }
        const int q = fdiv(by_reso, l);
        const long long nb = (long long)q + ((l - q * reso) ? 1 : 0);   // repeat.hpp:32-37
        v[0] = nb;
        // most runs of >= minbins windows a read can hold
        v[1] = nb + 1 < (1LL << 31) && minbins < INT32_MAX ? (long long)fdiv(by_mb1, (int)(nb + 1)) : (nb + 1) / ((long long)minbins + 1);
        if (nb > long_windows) v[1] += 2 * ((nb + piece_w - 1) / piece_w);   // + two runs per piece that touch its edges
        v[2] = fdiv(by_L, l) + 2;                                // chop.hpp:209-223
    }
};

template <int K> struct CountLoader {
    const int32_t *c[K];
    __device__ void operator()(long long i, long long (&v)[K]) const
    {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = c[k][i];
    }
};

// What the host reads back goes straight into its page-locked block (device-visible host memory): a copy command per
// few bytes cost ~25 us each on the device timeline (three of them ahead of the pass's host wait).  Stamped lines (finalize.hpp):
// run_pass looks for them itself instead of sleeping in the runtime's wait (as raft_hip_finish does for the pass's end).
constexpr int kInspWords = (int)(sizeof(InspectOut) / 8), kGuessWords = (int)(sizeof(GuessOut) / 8);
constexpr int kSizesWords = 3 + 2 + kInspWords + kGuessWords;      // scan totals; err_flags | pad, err_index; InspectOut; GuessOut
static_assert(kSizesWords <= 48 && stamped_lines(kSizesWords) * 8 <= 96, "the sizes block outgrew its place");
constexpr int kPackCountWord = 100;   // (raft_hip_pack's count of listed windows: a word of the block outside the stamped lines)
__global__ void publish_sizes_kernel(const long long *scan_totals, const Ctrl *ctrl, long long *host, long long seq)
{
    const long long *c8 = reinterpret_cast<const long long *>(ctrl);
    const long long *in = reinterpret_cast<const long long *>(&ctrl->insp), *gu = reinterpret_cast<const long long *>(&ctrl->guess);
    publish_stamped(host, [&](int i) { return i < 3 ? scan_totals[i] : i < 5 ? c8[i - 3] : i < 5 + kInspWords ? in[i - 5] : gu[i - 5 - kInspWords]; },
                    kSizesWords, seq, (int)threadIdx.x);
    __threadfence_system();
}

// The pass's last kernel: one wave copies the control block -- everything raft_hip_finish reports -- into the context's page-locked
// block, stamped with the pass's number (raft_hip_finish looks for it itself instead of sleeping in the runtime's wait, whose
// wake-up is 20-30 us of a pass that may take 200), and then clears the block and the hand-out counters for the NEXT pass: the
// one-wave launch that did that at the head of every pass (clear_ctrl_kernel) is only needed for a context's first pass now.
__global__ __launch_bounds__(64) void publish_and_clear_kernel(TailPublish tp, long long *ctrl_words, int32_t *wave_ctr, int word_err_index, int word_insp_err_index)
{
    const int t = (int)threadIdx.x;
    publish_stamped(tp.host_block, [&](int i) { return reinterpret_cast<const volatile long long *>(tp.ctrl_words)[i]; }, tp.n_ctrl_words, tp.pass_seq, t);
    __builtin_amdgcn_s_waitcnt(0x0F70);           // (every lane has its words: nothing below can overtake the reads)
    __threadfence_system();
    if (t < tp.n_ctrl_words) ctrl_words[t] = (t == word_err_index || t == word_insp_err_index) ? -1LL : 0LL;
    if (t < kWaveCounters) wave_ctr[t * kCtrStride] = 0;
}
__global__ void clear_ctrl_kernel(Ctrl *ctrl, int32_t *wave_ctr)
{
    constexpr int kWords = (int)(sizeof(Ctrl) / 8);
    if ((int)threadIdx.x < kWords) reinterpret_cast<long long *>(ctrl)[threadIdx.x] = 0;
    if ((int)threadIdx.x < kWaveCounters) wave_ctr[threadIdx.x * kCtrStride] = 0;
    __syncthreads();
    if (threadIdx.x == 0) { ctrl->err_index = -1; ctrl->insp.err_index = -1; }
}

__global__ void selftest_kernel(const int *in, int *out_dpp, int *out_shfl, unsigned long long *ballots)
{
    const int v = in[threadIdx.x];
    out_dpp[threadIdx.x] = wave_incl_scan_add(v);
    out_shfl[threadIdx.x] = wave_incl_scan_add_shfl(v);
    const unsigned long long b = __ballot(v & 1);
    if ((threadIdx.x & 63) == 0) ballots[threadIdx.x >> 6] = b;
}


} // namespace

void raft::launch_rebase_ids(hipStream_t st, int32_t *ids, long long n, int32_t base)
{
    hipLaunchKernelGGL(rebase_ids_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, ids, n, base);
}
void raft::launch_add_base(hipStream_t st, long long *a, long long n, long long base)
{
    hipLaunchKernelGGL(add_base_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, st, a, n, base);
}

namespace raft {

// The sides of a record stream in any order, sorted by read (bucket.hpp): o_rid / o_s / o_e hold every read's intervals
// together, reads in index order; off[r] says where read r's begin, off[n_reads] how many there are.
// What the two sorts share.  Before: the list of long runs of reads without intervals, emptied, and the bits of a key; after: the
// offsets of those reads, filled in from the list.
static int sides_begin(raft_hip_ctx *c, hipStream_t st, int32_t n_reads, int *bits)
{
    HIP_TRY(c, c->gaps.ensure(sizeof(GapList)));
    HIP_TRY(c, hipMemsetAsync(c->gaps.p, 0, 8, st));
    *bits = 1;
    while (*bits < 32 && (1LL << *bits) <= (long long)n_reads) ++*bits;            // keys 0 .. n_reads (the sides that do not exist)
    return RAFT_HIP_OK;
}
static int sides_end(raft_hip_ctx *c, hipStream_t st, long long *off)
{
    hipLaunchKernelGGL(fill_gaps_kernel, dim3(64), dim3(256), 0, st, c->gaps.as<GapList>(), off);
    HIP_TRY(c, hipGetLastError());
    return RAFT_HIP_OK;
}

int sort_sides(raft_hip_ctx *c, hipStream_t st, long long n_rec, int32_t n_reads, int symmetric, const int32_t *d_qid, const int32_t *d_qs,
               const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te, long long cap_iv, int32_t *o_rid, int32_t *o_s,
               int32_t *o_e, long long *off, int32_t *err_flags, long long *err_index)
{
    HIP_TRY(c, c->rs_k0.ensure((size_t)cap_iv * 4)); HIP_TRY(c, c->rs_k1.ensure((size_t)cap_iv * 4));
    HIP_TRY(c, c->rs_v0.ensure((size_t)cap_iv * 8)); HIP_TRY(c, c->rs_v1.ensure((size_t)cap_iv * 8));
    int bits = 1;
    { const int rc = sides_begin(c, st, n_reads, &bits); if (rc != RAFT_HIP_OK) return rc; }
    hipLaunchKernelGGL(expand_sides_kernel, dim3(grid_for(n_rec, 256, 256 * 32)), dim3(256), 0, st, n_rec, n_reads, symmetric, d_qid, d_qs, d_qe, d_tid, d_ts, d_te,
                       c->rs_k0.as<uint32_t>(), c->rs_v0.as<unsigned long long>(), err_flags, err_index);
    uint32_t *k_sorted = c->rs_k1.as<uint32_t>();
    unsigned long long *v_sorted = c->rs_v1.as<unsigned long long>();
    {   // sort_pairs.hpp: LSD radix sort, eight bits per pass, every store part of a run (hand-written since round 5: no library call on this path)
        HIP_TRY(c, c->sort_tmp.ensure(rs_tmp_bytes<unsigned long long>(cap_iv)));
        bool in_b = false;
        HIP_TRY(c, radix_sort_by_key<unsigned long long>(st, c->rs_k0.as<uint32_t>(), c->rs_v0.as<unsigned long long>(), c->rs_k1.as<uint32_t>(),
                                                         c->rs_v1.as<unsigned long long>(), cap_iv, bits, c->sort_tmp.p, &in_b));
        if (!in_b) { k_sorted = c->rs_k0.as<uint32_t>(); v_sorted = c->rs_v0.as<unsigned long long>(); }
    }
    hipLaunchKernelGGL(unzip_sorted_kernel, dim3(grid_for(cap_iv, 256, 256 * 32)), dim3(256), 0, st, cap_iv, n_reads, k_sorted, v_sorted,
                       o_rid, o_s, o_e, off, c->gaps.as<GapList>());
    return sides_end(c, st, off);
}

// ... the same as window records (bucket.hpp, round 5): o_win holds every read's records together, one word each (first window | one
// past the last << 16), off[] where every read's begin -- the pileup kernel's window-record input with one run.  8 bytes per side
// through the sort instead of 12.  A side whose windows need more than 16 bits raises kErrWide (raft_hip_finish runs the pass again
// with the coordinate route).
static int sort_sides_win(raft_hip_ctx *c, hipStream_t st, long long n_rec, int32_t n_reads, int symmetric, const int32_t *d_qid, const int32_t *d_qs,
                          const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te, long long cap_iv, uint32_t *o_win,
                          long long *off, int32_t *err_flags, long long *err_index)
{
    HIP_TRY(c, c->rs_v0.ensure((size_t)cap_iv * 8)); HIP_TRY(c, c->rs_v1.ensure((size_t)cap_iv * 8));
    int bits = 1;
    { const int rc = sides_begin(c, st, n_reads, &bits); if (rc != RAFT_HIP_OK) return rc; }
    HIP_TRY(c, c->sort_tmp.ensure(rs_items_tmp_bytes(cap_iv)));
    bool in_b = false;
    // (the first pass makes its items from the columns: no expansion kernel, no 16 bytes per side written and read back)
    const SideSource src{(long long)n_rec, n_reads, symmetric, make_fast_div(c->prm.reso), d_qid, d_qs, d_qe, d_tid, d_ts, d_te, err_flags, err_index};
    HIP_TRY(c, radix_sort_items(st, src, c->rs_v0.as<unsigned long long>(), c->rs_v1.as<unsigned long long>(), cap_iv, bits, c->sort_tmp.p, &in_b));
    const unsigned long long *sorted = in_b ? c->rs_v1.as<unsigned long long>() : c->rs_v0.as<unsigned long long>();
    hipLaunchKernelGGL(unzip_items_kernel, dim3(grid_for(cap_iv, 256, 256 * 32)), dim3(256), 0, st, cap_iv, n_reads, sorted, o_win, off, c->gaps.as<GapList>());
    return sides_end(c, st, off);
}

// Waits until the stamped lines (finalize.hpp publish_stamped) carry number `seq`.  The host looks for the number itself for up to
// `budget_ms` (the runtime's wait sleeps, and waking up costs 20-30 us) and falls back to the runtime's wait on `st` -- which is
// also what reports a device fault.  A pipeline lane does not spin at all -- its thread shares the host's cores with the other
// lanes, the tokeniser's and the formatter's workers, and its pass is a tenth of its transfers --, and RAFT_NO_SPIN=1 says so for
// every context.  *seen: the number was seen without the runtime.
static int wait_stamped(raft_hip_ctx *c, const volatile long long *lines, int n_words, long long seq, int budget_ms, hipStream_t st, bool *seen)
{
    *seen = false;
    if (budget_ms > 0 && !c->is_lane && getenv("RAFT_NO_SPIN") == nullptr) {
        const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(budget_ms);
        for (int it = 0; !(*seen = stamped_seen(lines, n_words, seq)); ++it)
            if ((it & 255) == 255 && std::chrono::steady_clock::now() > t_end) break;
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!*seen) HIP_TRY(c, hipStreamSynchronize(st));
    return RAFT_HIP_OK;
}

// ---- run_pass, phase by phase.  Each phase reads and writes one plain PassPlan and returns an engine error code.

// The environment switches of a pass.  They are read at EVERY pass (tests flip them inside one process), and this is the one place
// that lists them.  Read elsewhere: RAFT_NO_SPIN by both host waits (wait_stamped); once per process RAFT_HOST_CLOCK (hc_mark)
// and RAFT_PLACEMENT_TRIALS (engine_ctx.hpp); RAFT_COV_WIDTH at raft_hip_create.
struct PassSwitches {
    bool no_window_kernel;    // RAFT_NO_WINDOW_KERNEL: window records are unpacked to coordinate columns however few the runs
    bool always_inspect;      // RAFT_ALWAYS_INSPECT: no pass verifies in its kernels (A/B measurements; bench.py times both forms)
    bool no_hint;             // RAFT_NO_HINT: the caller's window count is ignored
    bool always_clear;        // RAFT_ALWAYS_CLEAR: clear_ctrl_kernel at the head of every pass
    bool no_speculate;        // RAFT_NO_SPECULATE: nothing is built on the last pass's shape
    bool no_fused_head;       // RAFT_NO_FUSED_HEAD: a pass sized by the caller's count scans and cuts in separate launches
    bool no_keep_geometry;    // RAFT_NO_KEEP_GEOMETRY: a speculative pass scans the geometry again
    bool no_radix_sort;       // RAFT_NO_RADIX_SORT: the counting sort whatever the size
    bool no_bucket_windows;   // RAFT_NO_BUCKET_WINDOWS: the general bucketing sorts coordinate pairs
    int extra_cap;            // RAFT_EXTRA_CAP (tests: tiles without slots of their own); -1: not set
    int deep_min;             // RAFT_DEEP_MIN (tests: ordinary tiles through pileup_deep_kernel); 0: not set
    bool graded_off;          // RAFT_GRADED_QUANTUM=0: every set gets a uniform quantum, as until round 6
    long long graded_min;     // RAFT_GRADED_MIN (tests: small sets under the graded quantum): graded from this many tiles' worth of windows on; -1: not set
};
static PassSwitches read_switches()
{
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    PassSwitches s{};
    s.no_window_kernel = on("RAFT_NO_WINDOW_KERNEL"); s.always_inspect = on("RAFT_ALWAYS_INSPECT"); s.no_hint = on("RAFT_NO_HINT");
    s.always_clear = on("RAFT_ALWAYS_CLEAR"); s.no_speculate = on("RAFT_NO_SPECULATE"); s.no_fused_head = on("RAFT_NO_FUSED_HEAD");
    s.no_keep_geometry = on("RAFT_NO_KEEP_GEOMETRY"); s.no_radix_sort = on("RAFT_NO_RADIX_SORT"); s.no_bucket_windows = on("RAFT_NO_BUCKET_WINDOWS");
    const char *ec = getenv("RAFT_EXTRA_CAP"), *dm = getenv("RAFT_DEEP_MIN");
    s.extra_cap = ec ? std::max(0, atoi(ec)) : -1;
    s.deep_min = dm ? std::max(1, atoi(dm)) : 0;
    const char *gq = getenv("RAFT_GRADED_QUANTUM"), *gm = getenv("RAFT_GRADED_MIN");
    s.graded_off = gq && atoi(gq) == 0;
    s.graded_min = gm ? std::max(0LL, atoll(gm)) : -1;
    return s;
}

struct PassPlan {
    PassSwitches sw;
    hipStream_t st;
    Ctrl *ctrl;
    std::chrono::steady_clock::time_point hc_t0;
    // the input as the kernels get it (resolve_input, open_pass): columns after substitution, the offsets and runs of a grouped pass
    int32_t n_reads;
    int64_t n_rec;
    long long N;                      // n_reads
    const int32_t *d_len, *d_qid, *d_qs, *d_qe, *d_tid, *d_ts, *d_te;
    const uint32_t *d_win;
    const long long *eff_off;
    GroupedOff grp;
    int32_t eff_runs;
    // the decisions
    bool grouped;                     // built on the caller's offsets
    bool lean;                        // window records go to the pileup kernel as they are
    bool merge;                       // more runs than the pileup kernels take: merged into one first
    bool expand;                      // no query column: the ids are rebuilt from the offsets
    bool spec;                        // verifies in its kernels
    bool speculate;                   // built on the shape the context's last pass found
    bool known;                       // the host knows the sizes before anything has run
    bool keep_geom;                   // the per-read geometry the context holds is kept
    bool no_wait;                     // sized by the caller's window count
    bool want_guess;                  // the sorted-segment path is possible
    bool fast;                        // the pileup reads the columns as they are: a handful of sorted runs
    bool table_ok;                    // the samples index the stream the pass is built on
    bool bwin;                        // the general bucketing hands the pileup kernel window records
    bool parked;                      // an input error the host saw on the way ended the pass (park_input_error)
    bool look_again;                  // detecting, and not a handful of sorted runs: the pass begins again, looking at every record
    int ow;                           // the width the pileup kernel writes cov[] in (int32, or its transfer encodings: pileup_wave.hpp OW)
    // the sizes
    long long B, RU, CU;              // windows, reserved raw-repeat slots, marker capacity
    Quantum qz;
    long long n_tiles, extra_cap, d4_tiles;
    int nb_scan, tail_blocks, n_waves;
    long long *scan_totals;
    long long h[kSizesWords];         // the sizes hand-over, taken out of its stamped lines (find_sizes)
    InspectOut *hi() { return reinterpret_cast<InspectOut *>(h + 5); }
    GuessOut *hg() { return reinterpret_cast<GuessOut *>(h + 5 + kInspWords); }
    // the interval source
    SegStarts sb;
    const long long *seg_end_dev;
    int symmetric, n_desc;
    long long desc[kMaxSeg];
};

// The quantum a pass over B windows runs on (choose_quantum; reset_and_decide asks for the remembered shape's B, before the pass has
// its own): by the context's tuning, the environment's switches and B alone.
static Quantum quantum_for(const raft_hip_ctx *c, const PassSwitches &sw, long long B)
{
    const long long q3 = 3LL * (kTileCap / 128) * 128, q1 = (kTileCap / 128) * 128;
    const int Q = c->tile_q ? std::max(256, c->tile_q) : (int)std::max(2 * q1, std::min(q3, (B / (2LL * wave_grid_waves(true))) / 128 * 128));
    // A set with many tiles per worker gets a GRADED quantum (quantum.hpp Quantum): most of each eighth of the set in ranges of
    // eight tiles' worth, its last tenth in ranges of two -- half the boundaries tile_desc_kernel has to look up, and the kernel's end
    // waits for a short draw.  (RAFT_GRADED_QUANTUM=0: uniform, as until round 6.  RAFT_GRADED_MIN=<n>: graded from n tiles' worth
    // of windows on -- 0: always -- so that tests reach this path with small sets.)
    const long long graded_min = sw.graded_min >= 0 ? sw.graded_min : 64LL * wave_grid_waves(true);
    const bool graded = !c->tile_q && !sw.graded_off && B / kTileCap >= graded_min && (B + 7) / 8 + 128 < (1LL << 31);
    return graded ? graded_quantum(B, 8 * (int)q1, 2 * (int)q1, 0.9) : uniform_quantum(Q);
}
// (the kind, and for a graded one everything graded_quantum returned)
static bool same_quantum(const Quantum &a, const Quantum &b)
{
    return a.q == b.q && a.share == b.share && a.per_share == b.per_share && a.n_long == b.n_long && a.q_long == b.q_long && a.q_short == b.q_short;
}

// (RAFT_HOST_CLOCK=1: where the host is, us after entering, when it has issued what -- a speculative pass over an eighth of the
// bench set is issued in 26 us, 2-3 us a launch: profiles/r06_host_clock.txt)
static void hc_mark(const PassPlan &P, const char *what)
{
    static const bool host_clock = getenv("RAFT_HOST_CLOCK") != nullptr;
    if (host_clock) fprintf(stderr, "[host] %-18s %7.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - P.hc_t0).count());
}

// An error in the input that the host has seen on the way: kept for raft_hip_finish, and the pass ends here with its events recorded.
static int park_input_error(raft_hip_ctx *c, PassPlan &P, int32_t flags, long long index)
{
    c->pending_err = code_from_flags(flags);
    c->pending_err_index = index;
    c->ran = true;
    HIP_TRY(c, hipEventRecord(c->ev_pile0, P.st)); HIP_TRY(c, hipEventRecord(c->ev_pile1, P.st));
    HIP_TRY(c, hipEventRecord(c->ev_pass1, P.st));
    P.parked = true;
    return RAFT_HIP_OK;
}

// Parameter checks, which form of input this is, and the columns the kernels will read in place of the caller's.
static int resolve_input(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &in, PassPlan &P)
{
    const int32_t n_reads = P.n_reads = in.n_reads;
    const int64_t n_rec = P.n_rec = in.n_rec;
    P.N = n_reads;
    P.d_len = in.len; P.d_qid = in.col[0]; P.d_qs = in.col[1]; P.d_qe = in.col[2]; P.d_tid = in.col[3]; P.d_ts = in.col[4]; P.d_te = in.col[5];
    P.grouped = in.rec_off != nullptr;
    P.d_win = in.win;
    if (n_reads < 0 || n_rec < 0) return RAFT_HIP_ERR_PARAM;
    if (n_reads > 0 && !P.d_len) return RAFT_HIP_ERR_PARAM;
    if (P.grouped && (in.n_runs < 1 || in.n_runs > kMaxRuns || c->prm.symmetric_mode != 1)) return RAFT_HIP_ERR_PARAM;
    if (P.d_win && (!P.grouped || c->prm.reso > 32767)) return RAFT_HIP_ERR_PARAM;   // (65535 windows * reso stays inside int32 where they are unpacked)
    // more runs than the pileup kernels take: merged into one on the device first (bucket.hpp merge_runs_kernel)
    P.merge = P.grouped && in.n_runs > kMaxSeg && n_rec > 0;
    P.eff_runs = P.grouped ? (in.n_runs > kMaxSeg ? 1 : in.n_runs) : 0;
    if (n_rec > 0 && ((!P.d_qid && !P.grouped) || ((!P.d_qs || !P.d_qe) && !P.d_win))) return RAFT_HIP_ERR_PARAM;
    if (n_reads == INT32_MAX) return RAFT_HIP_ERR_TOO_LARGE;
    if (n_rec >= (1LL << 29)) return RAFT_HIP_ERR_TOO_LARGE;   // interval byte offsets are 32-bit (2 sides per record at most)
    HIP_TRY(c, hipSetDevice(c->device));
    P.st = c->stream;
    // window records go to the pileup kernel's own instantiation (pileup_wave.hpp IN = 1) where the runs are few; anything else gets
    // coordinate columns that fall into the same windows (bucket.hpp unpack_windows_kernel) and takes the paths those have
    P.lean = P.d_win && n_rec > 0 && !P.merge && P.eff_runs <= kWinMaxRuns && !c->force_bucket && !P.sw.no_window_kernel;
    if (P.d_win && !P.lean && n_rec > 0) {
        HIP_TRY(c, c->u_s.ensure((size_t)n_rec * 4));
        HIP_TRY(c, c->u_e.ensure((size_t)n_rec * 4));
        P.d_qs = c->u_s.as<int32_t>(); P.d_qe = c->u_e.as<int32_t>();
    }
    if (P.merge) {
        HIP_TRY(c, c->b_rid.ensure((size_t)n_rec * 4));
        HIP_TRY(c, c->b_s.ensure((size_t)n_rec * 4));
        HIP_TRY(c, c->b_e.ensure((size_t)n_rec * 4));
        HIP_TRY(c, c->m_off.ensure((size_t)(n_reads + 1LL) * 8));
    } else if (n_rec > 0 && P.grouped && !P.d_qid && !P.lean) {      // no query column: the ids are rebuilt from the offsets
        HIP_TRY(c, c->exp_qid.ensure((size_t)n_rec * 4));
        P.d_qid = c->exp_qid.as<int32_t>();
        P.expand = true;
    }
    if (n_rec > 0 && (!P.d_tid || !P.d_ts || !P.d_te)) {
        // symmetric_mode = 1: the target columns are never read (query sides only, no detection) and may be omitted
        if (c->prm.symmetric_mode != 1) return RAFT_HIP_ERR_PARAM;
        P.d_tid = P.d_qid; P.d_ts = P.d_qs; P.d_te = P.d_qe;
    }
    return RAFT_HIP_OK;
}

// The context's state of the last pass goes, and everything is decided that can be decided before the device has been asked: which
// form of a pass this is.  No HIP call in here.
static void reset_and_decide(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &in, bool verify_in_kernels, PassPlan &P)
{
    c->ran = false; c->finished = false; c->pending_err = RAFT_HIP_OK; c->pending_err_index = -1; c->packed_width = 0; c->seq_armed = false;
    c->cov_valid = false; c->pass_width = 4; c->n_exc = 0; c->exc_sorted = false; c->spec_scanned = false;
    c->args = in;
    // (a detecting context assumes a symmetric PAF -- hifiasm's shape -- until a pass of its own has found otherwise)
    P.spec = !P.grouped && verify_in_kernels && !P.sw.always_inspect && P.n_rec > 1 && !c->force_bucket &&
             (c->prm.symmetric_mode == 1 || (c->prm.symmetric_mode < 0 && c->assume_sym));
    c->spec = P.spec;
    c->grouped = P.grouped;
    memset(&c->sum, 0, sizeof c->sum);
    c->sum.n_reads = P.n_reads; c->sum.n_records = P.n_rec; c->sum.high_cov = c->high_cov; c->sum.error_index = -1;
    P.ow = c->out_width;
    // a grouped pass whose caller announced the window count needs nothing back from the device on the way
    P.no_wait = P.grouped && in.hint_bins >= 0 && !P.sw.no_hint;
    c->no_wait = P.no_wait;
    P.hc_t0 = std::chrono::steady_clock::now();
    P.want_guess = !P.grouped && P.n_rec > 1 && c->prm.symmetric_mode != 0 && !c->force_bucket;   // (the sorted-segment path is possible)
    // ---- A pass whose sizes the host knows before anything has run needs no wait on the way, and its head is THREE launches
    // (round 6): [geometry scan, first half | run guess] -> [geometry scan, second half + the per-read work of tile_first_kernel +
    // the check of what was assumed] -> tile_desc_kernel.  Two ways to know:
    //  * the caller of a grouped pass announced its window count (no_wait, since round 3);
    //  * SPECULATION: the context's last pass over plain columns went the sorted-run way, and this one has the same shape -- reads,
    //    records, column addresses, parameters.  It is built on what that pass found (windows, reserved slots, where the runs end)
    //    and every kernel that relies on it checks it: the scan's totals against the assumed ones, the sampled run ends against
    //    the assumed ones (kErrHint: the later kernels return at once and raft_hip_finish runs the pass again the long way).
    //    A streaming caller that hands over batch after batch through the same buffers gets the long way once.
    const bool shape_fits = c->shape.valid && c->shape.n_reads == P.n_reads && c->shape.n_rec == P.n_rec && c->shape.len == (const void *)P.d_len &&
                            c->shape.qid == (const void *)P.d_qid && c->shape.reso == c->prm.reso && c->shape.minbins == c->minbins &&
                            c->shape.interval_length == c->prm.interval_length && c->shape.symmetric_mode == c->prm.symmetric_mode &&
                            c->shape.tile_q == c->tile_q && same_quantum(c->shape.qz, quantum_for(c, P.sw, c->shape.B));
    P.speculate = P.spec && shape_fits && P.N > 0 && !c->is_lane && !P.sw.no_speculate;
    P.known = P.N > 0 && (P.speculate || (P.no_wait && !P.sw.no_fused_head));
    c->speculated = P.speculate;
    if (P.speculate) c->sum.flags |= RAFT_HIP_SUM_SPECULATED;
    // (the geometry of the remembered pass, if nobody has written it since: engine_ctx.hpp geom_id.  RAFT_NO_KEEP_GEOMETRY=1: scanned again)
    P.keep_geom = P.speculate && !P.grouped && c->geom_id != 0 && c->shape.geom_id == c->geom_id && !P.sw.no_keep_geometry;
    if (!P.keep_geom) ++c->geom_id;
    else c->sum.flags |= RAFT_HIP_SUM_KEPT_GEOMETRY;
    // (a speculative pass that scans writes the geometry of the same reads afresh: raft_hip_finish lets the passes after it keep that
    // geometry once the pass has come through without an error flag or a re-run -- not before: a scan that met a negative length
    // has recorded it in len_seen)
    c->spec_scanned = P.speculate && !P.keep_geom;
    c->spec_geom_id = c->geom_id;
}

// The pass's first event, the buffers the head needs (sized by the input alone), a clear control block, and the caller's columns
// brought into the form the kernels take: window records unpacked, more than kMaxSeg runs merged.
static int open_pass(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &in, PassPlan &P)
{
    hipStream_t st = P.st;
    const int32_t n_reads = P.n_reads;
    const int64_t n_rec = P.n_rec;
    HIP_TRY(c, hipEventRecord(c->ev_pass0, st));
    hc_mark(P, "ev_pass0");
    HIP_TRY(c, c->ctrl.ensure(sizeof(Ctrl)));
    Ctrl *ctrl = P.ctrl = c->ctrl.as<Ctrl>();
    HIP_TRY(c, c->wave_ctr.ensure((size_t)kWaveCounters * kCtrStride * 4));
    P.nb_scan = std::max(scan_blocks(P.N), 1);
    HIP_TRY(c, c->scan_tmp.ensure(((size_t)P.nb_scan * 3 + 8) * sizeof(long long)));
    HIP_TRY(c, c->cov_off.ensure((size_t)(P.N + 1) * 8));
    HIP_TRY(c, c->rep_res_off.ensure((size_t)(P.N + 1) * 8));
    if (P.want_guess) HIP_TRY(c, c->samples.ensure((size_t)(kSamples + 2) * 4));
    HIP_TRY(c, c->len_seen.ensure((size_t)std::max(P.N, 1LL) * 4));
    // (the last pass's closing kernel has cleared the block behind its hand-over -- unless this is the context's first pass, the
    // last one did not get that far, or the stream is another)
    if (!c->ctrl_clean || c->clean_stream != st || P.sw.always_clear)
        hipLaunchKernelGGL(clear_ctrl_kernel, dim3(1), dim3(64), 0, st, ctrl, c->wave_ctr.as<int32_t>());      // (three fill commands before: ~5 us each on the device)
    c->ctrl_clean = false;
    if (P.d_win && !P.lean && n_rec > 0)
        hipLaunchKernelGGL(unpack_windows_kernel, dim3(grid_for(n_rec, 256, 256 * 16)), dim3(256), 0, st,
                           (long long)n_rec, P.d_win, c->prm.reso, c->u_s.as<int32_t>(), c->u_e.as<int32_t>());
    P.eff_off = in.rec_off;
    if (P.merge) {
        const long long stride = (long long)n_reads + 1;
        hipLaunchKernelGGL(check_offsets_kernel, dim3((unsigned)((n_reads + 1LL + 255) / 256)), dim3(256), 0, st, n_reads, in.n_runs, in.rec_off, stride,
                           (long long)n_rec, &ctrl->err_flags, &ctrl->err_index);
        hipLaunchKernelGGL(merge_runs_kernel, dim3(grid_for((n_reads + 64LL) / 64, 4, 256 * 16)), dim3(256), 0, st,
                           n_reads, in.n_runs, in.rec_off, stride, P.d_qs, P.d_qe, c->m_off.as<long long>(), c->b_rid.as<int32_t>(), c->b_s.as<int32_t>(),
                           c->b_e.as<int32_t>(), &ctrl->err_flags);
        P.d_qid = P.d_tid = c->b_rid.as<int32_t>(); P.d_qs = P.d_ts = c->b_s.as<int32_t>(); P.d_qe = P.d_te = c->b_e.as<int32_t>();
        P.eff_off = c->m_off.as<long long>();
    }
    if (P.grouped) {
        P.grp.off = P.eff_off; P.grp.stride = P.N + 1;
        for (int s2 = 0; s2 < kMaxSeg; ++s2) P.grp.adj[s2] = P.merge ? 0 : in.adj[s2];
    }
    return RAFT_HIP_OK;
}

// the per-read geometry scan: windows, reserved repeat slots, marker capacity (one scan, three sums)
static ReadPrepLoader prep_loader(raft_hip_ctx *c, const PassPlan &P)
{
    return ReadPrepLoader{P.d_len, c->prm.reso, c->minbins, c->prm.interval_length, kTileCap, kTileCap,
                          &P.ctrl->err_flags, &P.ctrl->err_index, make_fast_div(c->prm.reso),
                          make_fast_div(c->minbins < INT32_MAX ? c->minbins + 1 : 1), make_fast_div(c->prm.interval_length), c->len_seen.as<int32_t>()};
}
static ScanOut<3> prep_out(raft_hip_ctx *c)
{
    return ScanOut<3>{{c->cov_off.as<long long>(), c->rep_res_off.as<long long>(), nullptr}};   // (marker capacities: only their sum is used, to size the cut points' array)
}

// B, RU, CU: remembered, or from the caller's window count, or from the device -- the pass's only host wait.
static int find_sizes(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &in, PassPlan &P)
{
    hipStream_t st = P.st;
    Ctrl *ctrl = P.ctrl;
    const long long N = P.N;
    const int64_t n_rec = P.n_rec;
    // ---- two things have to be known before the host can size and launch the rest, and they run side by side:
    //  (main stream) what the record stream looks like -- sorted runs sampled by guess_runs_kernel and, unless the pass
    //      verifies in its kernels, every record by inspect_kernel: ids in range? the runs as sampled? mirror of record 0?
    //  (side stream) the per-read geometry: windows, reserved repeat slots, marker capacity (one scan, three sums).
    // (a grouped pass has nothing to find out about the stream: the scan runs on the main stream, nothing beside it)
    if (!P.known) {
        hipStream_t gst = P.grouped ? st : c->side_stream;
        if (!P.grouped) {
            HIP_TRY(c, hipEventRecord(c->ev_ifork, st));                    // (the control block is clear)
            HIP_TRY(c, hipStreamWaitEvent(gst, c->ev_ifork, 0));
        }
        exclusive_scan<ReadPrepLoader, 3>(gst, prep_loader(c, P), N, c->scan_tmp.as<long long>(), prep_out(c), &P.scan_totals);
        if (!P.grouped) HIP_TRY(c, hipEventRecord(c->ev_gjoin, gst));
        if (n_rec > 0 && !P.grouped) {
            if (P.want_guess)
                hipLaunchKernelGGL(guess_runs_kernel, dim3(kGuessBlocks), dim3(256), 0, st, (long long)n_rec, P.d_qid, &ctrl->guess,
                                   c->samples.as<int32_t>());
            if (!P.spec)
                hipLaunchKernelGGL(inspect_kernel, dim3(grid_for(n_rec / 4, 256, 256 * 8)), dim3(256), 0, st, (long long)n_rec, P.n_reads,
                                   c->prm.symmetric_mode < 0 ? 1 : 0, P.d_qid, P.d_qs, P.d_qe, P.d_tid, P.d_ts, P.d_te, &ctrl->insp);
        }
        if (!P.grouped) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_gjoin, 0));
    }
    if (P.speculate) {
        P.B = c->shape.B; P.RU = c->shape.RU; P.CU = c->shape.CU;
        P.hg()->n_desc = c->shape.n_desc;
        for (int i = 0; i < kMaxSeg; ++i) P.hg()->desc_pos[i] = c->shape.desc[i];
    } else if (P.no_wait) {
        // (the caller's count is compared with the scan's on the device: kErrHint stops the pass there, and raft_hip_finish runs
        // it again with the host wait)
        // sizes from the caller's window count: B as announced (checked on the device, kErrHint); bounds for the rest --
        // reserved raw-repeat slots sum_r ((w_r + 1) / (minbins + 1) + two per piece of a long read), markers sum_r (len_r / L + 2)
        const long long B = P.B = in.hint_bins;
        P.RU = (B + N) / ((long long)c->minbins + 1) + 4 * (B / kTileCap) + 4;
        P.CU = B / std::max(1, c->prm.interval_length / c->prm.reso) + 2 * N + 2;
        if (c->prm.interval_length < c->prm.reso) P.CU = B * ((long long)c->prm.reso / c->prm.interval_length + 1) + 2 * N + 2;
    } else {
        hipLaunchKernelGGL(publish_sizes_kernel, dim3(1), dim3(64), 0, st, P.scan_totals, ctrl, c->pinned_dev, ++c->sizes_seq);
        // the pass's only host wait: sizes + path choice (bounded by 2 ms of looking for the lines)
        const volatile long long *lines = reinterpret_cast<const volatile long long *>(c->pinned);
        bool seen = false;
        PHASE(wait_stamped(c, lines, kSizesWords, c->sizes_seq, 2, st, &seen));
        unstamp(lines, kSizesWords, P.h);
        P.B = P.h[0]; P.RU = P.h[1]; P.CU = P.h[2];
        const int32_t flags = reinterpret_cast<int32_t *>(P.h + 3)[0];
        if (flags) return park_input_error(c, P, flags, P.h[4]);
    }
    c->sum.n_bins = P.B; c->sum.total_windows = P.B;
    if (P.RU >= (1LL << 31)) return RAFT_HIP_ERR_TOO_LARGE;   // reserved raw-repeat slots are indexed with 32 bits in LDS
    return RAFT_HIP_OK;
}

// The quantum: boundaries at which a worker of the pileup kernel may begin (it cuts its tiles itself; tile_desc_kernel finds each
// boundary's first read, records and window).  Three tiles' worth (four until round 5: on the human-scale set the kernel likes
// short ranges -- 2.42 / 2.45 / 2.49 / 2.56 ms at two / three / four / eight tiles' worth in one context -- and tile_desc_kernel
// long ones; the pass is shortest at three, profiles/r05_quantum_sweep.txt).  Smaller sets keep the three tiles' worth down to
// two ranges per worker, and two tiles' worth below that: a draw is an atomic and two boundary records a worker waits for, and
// with five to fifteen tiles per worker those waits cost more than the kernel's last draws do (profiles/r06_quantum_small_sets.txt:
// an eighth of the human-scale set 0.424 -> 0.410 ms per step, 200 k reads 0.289 -> 0.276, 50 k reads 0.186 -> 0.178; until
// round 6 such sets were cut into eight ranges per worker or single tiles' worth).
static void choose_quantum(raft_hip_ctx *c, PassPlan &P)
{
    const long long B = P.B;
    P.qz = quantum_for(c, P.sw, B);
    if (P.qz.share) c->sum.flags |= RAFT_HIP_SUM_GRADED_RANGES;
    P.n_tiles = P.qz.n_ranges(B);
    // delta4: a tile lists windows in slots of its own, named by a tile id; the number bounds the ids that have slots (the tiles are
    // cut by the workers -- a tile is closed by a full array, 63 reads, a long read or the end of a range; ids are drawn 32 at a time;
    // a tile beyond them lists in the shared list)
    P.extra_cap = P.ow == kCovDelta4 ? 2 * P.n_tiles + 2 * (B / kTileCap) + P.N / 32 + 32LL * wave_grid_waves(true) + 1024 : 0;
    if (P.sw.extra_cap >= 0) P.extra_cap = P.sw.extra_cap;
    P.d4_tiles = P.n_tiles + P.extra_cap;             // (tile ids with slots of their own)
}

// Every buffer the rest of the pass writes, grown to the sizes just found.
static int ensure_buffers(raft_hip_ctx *c, PassPlan &P)
{
    const long long N = P.N, B = P.B, RU = P.RU, CU = P.CU, n_tiles = P.n_tiles;
    const int ow = P.ow;
    if (ow == 4) HIP_TRY(c, c->cov.ensure((size_t)std::max(B, 1LL) * 4));
    else {
        if (ow == kCovDelta4) {
            HIP_TRY(c, c->cov8.ensure((size_t)std::max(B, 1LL) / 2 + 16));
            HIP_TRY(c, c->cov_anchor.ensure(((size_t)std::max(B, 1LL) / kD4Block + 3) * 4));
        } else
            HIP_TRY(c, c->cov8.ensure((size_t)std::max(B, 1LL) * (size_t)ow + 16));
        const long long cap = std::max<long long>(c->exc_cap, std::max<long long>(4096, B / 64));
        HIP_TRY(c, c->exc_idx.ensure((size_t)cap * 8));
        HIP_TRY(c, c->exc_val.ensure((size_t)cap * 4));
        c->exc_cap = cap;
    }
    HIP_TRY(c, c->tile_first.ensure((size_t)(n_tiles + 1) * 4));
    if ((n_tiles + 1) * 8 >= (1LL << 31)) return RAFT_HIP_ERR_TOO_LARGE;   // boundary words are indexed with 32 bits
    HIP_TRY(c, c->tile_cuts.ensure((size_t)(n_tiles + 1) * sizeof(TileCut)));
    HIP_TRY(c, c->block_sums.ensure((size_t)256 * 8 * 16 * 2 * 4));
    for (DevBuf *b : {&c->rep_cnt, &c->cut_cnt, &c->frag_cnt}) HIP_TRY(c, b->ensure((size_t)std::max(N, 1LL) * 4));
    for (DevBuf *b : {&c->raw_key, &c->raw_s, &c->raw_e, &c->rep_s, &c->rep_e}) HIP_TRY(c, b->ensure((size_t)std::max(RU, 1LL) * 4));
    for (DevBuf *b : {&c->cuts, &c->frag_read, &c->frag_begin, &c->frag_end}) HIP_TRY(c, b->ensure((size_t)std::max(CU, 1LL) * 4));
    for (DevBuf *b : {&c->rep_off, &c->cut_off, &c->frag_off}) HIP_TRY(c, b->ensure((size_t)(N + 1) * 8));
    // the tail's sums: per workgroup of 256 reads four words from the count kernel, three of their prefix
    P.tail_blocks = (int)std::max<long long>(1, (N + 255) / 256);
    HIP_TRY(c, c->tail_buf.ensure((size_t)7 * P.tail_blocks * 8));
    if (ow == kCovDelta4) {
        HIP_TRY(c, c->exc_pidx.ensure((size_t)P.d4_tiles * kExcPerTile * 8));
        HIP_TRY(c, c->exc_pval.ensure((size_t)P.d4_tiles * kExcPerTile * 4));
        HIP_TRY(c, c->exc_tile_n.ensure((size_t)P.d4_tiles * 4));
    }
    HIP_TRY(c, c->deep_list.ensure((size_t)c->deep_cap * sizeof(DeepTile)));
    return RAFT_HIP_OK;
}

// The per-read geometry and each boundary's first read: the fused head where the sizes were known, tile_first_kernel behind the
// scan where they were not; the ids of a grouped pass without a query column.
static void launch_head(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &in, PassPlan &P)
{
    hipStream_t st = P.st;
    Ctrl *ctrl = P.ctrl;
    const long long N = P.N;
    if (P.known) {
        // the head in two launches (see reset_and_decide): the scan's first half with the run guess beside it, its second half with
        // the per-read work of tile_first_kernel riding on it
        const bool guess_too = !P.grouped && P.n_rec > 0 && P.want_guess;
        long long *partials = c->scan_tmp.as<long long>();
        P.scan_totals = partials + (long long)P.nb_scan * 3;
        GuessBeside gb{(long long)P.n_rec, P.d_qid, &ctrl->guess, c->samples.as<int32_t>()};
        if (P.keep_geom) {
            // ONE launch: the lengths against the ones the geometry was made from (kErrHint), the repeat counters cleared; the run guess beside it
            const int vb = (int)((N + kVerifyReads - 1) / kVerifyReads);
            hipLaunchKernelGGL((verify_lengths_kernel<GuessBeside>), dim3((unsigned)(vb + (guess_too ? kGuessBlocks : 0))), dim3(256), 0, st, P.n_reads, P.d_len,
                               c->len_seen.as<int32_t>(), c->rep_cnt.as<int32_t>(), &ctrl->err_flags, &ctrl->err_index, vb, gb);
        } else {
            const ReadPrepLoader prep_ld = prep_loader(c, P);
            hipLaunchKernelGGL((scan_partials_kernel<ReadPrepLoader, 3, GuessBeside>), dim3((unsigned)(P.nb_scan + (guess_too ? kGuessBlocks : 0))), dim3(kScanThreads), 0, st,
                               prep_ld, N, partials, P.nb_scan, gb);
            PrepPost pp{P.n_reads, P.qz, P.n_tiles, c->tile_first.as<int32_t>(), c->rep_cnt.as<int32_t>(), &ctrl->err_flags, &ctrl->err_index, P.grp, P.eff_runs,
                        (long long)P.n_rec, P.B, P.RU, P.CU};
            hipLaunchKernelGGL((scan_apply_kernel<ReadPrepLoader, 3, true, PrepPost>), dim3((unsigned)P.nb_scan), dim3(kScanThreads), 0, st, prep_ld, N, partials, P.scan_totals,
                               prep_out(c), pp);
        }
    } else
        hipLaunchKernelGGL(tile_first_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, st, P.n_reads,
                           c->cov_off.as<long long>(), P.qz, P.n_tiles, c->tile_first.as<int32_t>(), &ctrl->err_flags, &ctrl->err_index, P.grp,
                           P.eff_runs, (long long)P.n_rec, c->rep_cnt.as<int32_t>(), P.scan_totals, P.no_wait ? in.hint_bins : -1LL);
    hc_mark(P, "head launched");
    if (P.expand)
        hipLaunchKernelGGL(expand_ids_kernel, dim3(grid_for((N + 63) / 64 * P.eff_runs, 4, 256 * 16)),
                           dim3(256), 0, st, P.n_reads, P.eff_runs, P.grp, c->exp_qid.as<int32_t>(), &ctrl->err_flags);
}

// Where the pileup kernel's intervals will come from, as far as the host can say: the runs of the stream (as the offsets, the
// remembered shape, the samples or inspect_kernel name them), whether the targets' sides exist -- and what the context remembers of
// it for the next pass.  No launch on a clean stream; an input error inspect_kernel reported ends the pass here (an id out of range:
// after one look at the targets of the records before it, first_bad_target_kernel).
static int decide_source(raft_hip_ctx *c, PassPlan &P)
{
    const InspectOut *hi = P.hi();
    const GuessOut *hg = P.hg();
    P.symmetric = c->prm.symmetric_mode == 1 ? 1 : 0;
    if (P.grouped) {
        P.symmetric = 1;
        P.n_desc = P.eff_runs - 1;
    } else if (P.spec) {
        P.symmetric = 1;
        P.n_desc = hg->n_desc;
        for (int i = 0; i < std::min(P.n_desc, kMaxSeg); ++i) P.desc[i] = hg->desc_pos[i];
        P.table_ok = P.n_desc + 1 <= kMaxSeg;            // (the samples index the stream the pass is built on)
        if (c->prm.symmetric_mode < 0 && !P.table_ok) {  // detecting, and not a handful of sorted runs: look at every record after all
            P.look_again = true;
            return RAFT_HIP_OK;
        }
    } else if (P.n_rec > 0) {
        if (hi->err_flags) {
            long long index = hi->err_index;
            // inspect_kernel has looked at the query ids alone: unless the caller says the targets' sides do not exist, an earlier
            // record may name a target out of range (the control block's word still holds the index; the next pass clears it)
            if ((hi->err_flags & kErrReadId) && c->prm.symmetric_mode != 1 && index > 0 && index <= (long long)P.n_rec) {
                hipLaunchKernelGGL(first_bad_target_kernel, dim3(grid_for(index, 256, 1024)), dim3(256), 0, P.st, index, P.n_reads, P.d_tid, &P.ctrl->insp.err_index);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipMemcpyAsync(&index, &P.ctrl->insp.err_index, 8, hipMemcpyDeviceToHost, P.st));
                HIP_TRY(c, hipStreamSynchronize(P.st));
            }
            return park_input_error(c, P, hi->err_flags, index);
        }
        if (c->prm.symmetric_mode < 0) { P.symmetric = hi->sym_found ? 1 : 0; c->assume_sym = P.symmetric != 0; }
        P.n_desc = hi->n_desc;
        for (int i = 0; i < std::min(P.n_desc, kMaxSeg); ++i) P.desc[i] = hi->desc_pos[i];
        // the samples index the stream when the sampled run ends are exactly the ones the full pass found
        P.table_ok = P.want_guess && P.n_desc + 1 <= kMaxSeg && hg->n_desc == P.n_desc;
        for (int i = 0; P.table_ok && i < P.n_desc; ++i) {
            bool found = false;
            for (int j = 0; j < P.n_desc; ++j) found = found || hg->desc_pos[j] == P.desc[i];
            P.table_ok = found;
        }
    }
    c->sum.symmetric = P.symmetric;
    P.fast = P.n_rec > 0 && P.symmetric && !c->force_bucket && P.n_desc + 1 <= kMaxSeg;
    if (!P.grouped && P.spec && !P.speculate) {
        // what this pass found out on the way, for the next one over a stream of the same shape (see `speculate`); a pass that turns
        // out to have been built on a wrong guess takes it back (raft_hip_finish)
        c->shape.valid = P.fast && P.table_ok && P.N > 0;
        c->shape.n_reads = P.n_reads; c->shape.n_rec = P.n_rec; c->shape.len = P.d_len; c->shape.qid = P.d_qid;
        c->shape.reso = c->prm.reso; c->shape.minbins = c->minbins; c->shape.interval_length = c->prm.interval_length;
        c->shape.symmetric_mode = c->prm.symmetric_mode; c->shape.tile_q = c->tile_q; c->shape.qz = P.qz;
        c->shape.B = P.B; c->shape.RU = P.RU; c->shape.CU = P.CU; c->shape.n_desc = P.n_desc; c->shape.geom_id = c->geom_id;
        for (int i = 0; i < kMaxSeg; ++i) c->shape.desc[i] = i < P.n_desc ? P.desc[i] : 0;
    } else if (!P.speculate && !P.grouped) c->shape.valid = false;
    return RAFT_HIP_OK;
}

// The pileup kernels' arguments, but for the intervals (interval_source); delta4: the tiles' slots emptied.
static int fill_pileup_args(raft_hip_ctx *c, PassPlan &P, PileupArgs &pa)
{
    Ctrl *ctrl = P.ctrl;
    const int ow = P.ow;
    pa.read_len = P.d_len; pa.cov_off = c->cov_off.as<long long>();
    pa.n_tiles = P.n_tiles; pa.n_reads = P.n_reads;
    pa.reso = c->prm.reso; pa.high_cov = c->high_cov; pa.repeat_length = c->prm.repeat_length; pa.flank = c->prm.flanking_length;
    pa.cov = ow == 4 ? c->cov.as<int32_t>() : nullptr;
    pa.tile_batch = cov_line_bit(pa.cov);    // (the rest of the word: launch_pileup)
    pa.covp = ow == 4 ? nullptr : c->cov8.p; pa.n_exc = &ctrl->n_exc; pa.exc_cap = c->exc_cap;
    pa.cov_anchor = ow == kCovDelta4 ? c->cov_anchor.as<int32_t>() : nullptr; pa.d4_shift = c->d4_shift;
    if (ow == kCovDelta4) {
        HIP_TRY(c, hipMemsetAsync(c->exc_tile_n.p, 0, (size_t)P.d4_tiles * 4, P.st));
        pa.exc_pidx = c->exc_pidx.as<long long>(); pa.exc_pval = c->exc_pval.as<int32_t>(); pa.exc_tile_n = c->exc_tile_n.as<int32_t>();
    }
    pa.exc_idx = c->exc_idx.as<long long>(); pa.exc_val = c->exc_val.as<int32_t>();
    pa.rep_res_off = c->rep_res_off.as<long long>(); pa.rep_cnt = c->rep_cnt.as<int32_t>();
    pa.raw_key = c->raw_key.as<int32_t>(); pa.raw_s = c->raw_s.as<int32_t>(); pa.raw_e = c->raw_e.as<int32_t>();
    pa.block_sums = c->block_sums.as<long long>(); pa.err_flags = &ctrl->err_flags; pa.err_index = &ctrl->err_index;
    pa.tile_counter = c->wave_ctr.as<int32_t>(); pa.slow_counter = &ctrl->slow_next;
    // (a speculative pass over a stream whose last pass listed no deep tile does not launch the side kernel: 4 us of a 0.4 ms pass; a
    // tile that is deep after all finds no room in the list, and raft_hip_finish runs the pass again the long way)
    c->deep_skipped = P.speculate && !c->shape.had_deep && P.sw.deep_min == 0;
    pa.deep_list = c->deep_list.p; pa.n_deep = &ctrl->n_deep; pa.deep_cap = c->deep_skipped ? 0 : (int32_t)std::min<long long>(c->deep_cap, INT32_MAX);
    pa.deep_min = 32768; pa.deep_rep_total = &ctrl->totals[1];
    if (P.sw.deep_min) pa.deep_min = P.sw.deep_min;     // (tests: ordinary tiles through pileup_deep_kernel)
    {   // n / reso as mulhi + shift, exact for 0 <= n < 2^31: with L = ceil(log2 reso) and
        // m = floor(2^(31+L) / reso) + 1 (< 2^32), n / reso == (n * m) >> (31 + L) == mulhi(n, m) >> (L - 1)
        const unsigned d = (unsigned)c->prm.reso;
        if (d == 1) { pa.div_magic = 0; pa.div_shift = -1; }
        else {
            int L = 0;
            while ((1ull << L) < d) ++L;
            pa.div_magic = (uint32_t)((1ull << (31 + L)) / d + 1ull);
            pa.div_shift = L - 1;
        }
    }
    return RAFT_HIP_OK;
}

// The general interval source: the sides of a record stream in any order, bucketed by read -- counting sort, or for large inputs a
// radix sort of coordinate pairs (sort_sides) or of window records (sort_sides_win).
static int bucket_sides(raft_hip_ctx *c, PassPlan &P, PileupArgs &pa)
{
    hipStream_t st = P.st;
    Ctrl *ctrl = P.ctrl;
    const long long N = P.N;
    const int64_t n_rec = P.n_rec;
    const int32_t n_reads = P.n_reads;
    const int symmetric = P.symmetric;
    const long long cap_iv = symmetric ? (long long)n_rec : 2 * (long long)n_rec;
    HIP_TRY(c, c->b_cnt.ensure((size_t)std::max(N, 1LL) * 4));
    HIP_TRY(c, c->b_off.ensure((size_t)(N + 1) * 8));
    HIP_TRY(c, c->b_rid.ensure((size_t)cap_iv * 4));
    HIP_TRY(c, c->b_s.ensure((size_t)cap_iv * 4));
    HIP_TRY(c, c->b_e.ensure((size_t)cap_iv * 4));
    // large inputs are sorted, not scattered (bucket.hpp): the counting sort's random 12-byte writes took 87 ms for 2.9e8
    // shuffled records; it stays for small inputs, where its three launches cost less than the sort's
    // (... and for a symmetric stream of a few sorted runs that is sent here all the same -- force_bucket, A/B: its scatter is local)
    const bool parted = cap_iv >= (1LL << 20) && (!symmetric || P.n_desc + 1 > kMaxSeg) && !P.sw.no_radix_sort;
    // ... and as window records where the wave kernel runs and a window index fits 16 bits: 8 bytes per side through the sort,
    // the kernel's leanest input behind it
    P.bwin = parted && c->prm.reso <= 32767 && !c->no_bucket_win && !P.sw.no_bucket_windows;
    if (P.bwin) {
        PHASE(sort_sides_win(c, st, (long long)n_rec, n_reads, symmetric, P.d_qid, P.d_qs, P.d_qe, P.d_tid, P.d_ts, P.d_te, cap_iv,
                             c->b_s.as<uint32_t>(), c->b_off.as<long long>(), &ctrl->err_flags, &ctrl->err_index));
    } else if (parted) {
        PHASE(sort_sides(c, st, (long long)n_rec, n_reads, symmetric, P.d_qid, P.d_qs, P.d_qe, P.d_tid, P.d_ts, P.d_te, cap_iv,
                         c->b_rid.as<int32_t>(), c->b_s.as<int32_t>(), c->b_e.as<int32_t>(), c->b_off.as<long long>(),
                         &ctrl->err_flags, &ctrl->err_index));
    } else {
        HIP_TRY(c, hipMemsetAsync(c->b_cnt.p, 0, (size_t)std::max(N, 1LL) * 4, st));
        const unsigned grid = (unsigned)std::min<long long>((n_rec + 255) / 256, 8192);
        hipLaunchKernelGGL(bucket_hist_kernel, dim3(grid), dim3(256), 0, st, (long long)n_rec, n_reads, symmetric, P.d_qid,
                           P.d_tid, c->b_cnt.as<int32_t>(), &ctrl->err_flags, &ctrl->err_index);
        {
            CountLoader<1> ld{{c->b_cnt.as<int32_t>()}};
            ScanOut<1> so{{c->b_off.as<long long>()}};
            exclusive_scan<CountLoader<1>, 1>(st, ld, N, c->scan_tmp.as<long long>(), so);
        }
        HIP_TRY(c, hipMemsetAsync(c->b_cnt.p, 0, (size_t)std::max(N, 1LL) * 4, st)); // reused as the scatter cursor
        hipLaunchKernelGGL(bucket_scatter_kernel, dim3(grid), dim3(256), 0, st, (long long)n_rec, n_reads, symmetric, P.d_qid,
                           P.d_qs, P.d_qe, P.d_tid, P.d_ts, P.d_te, c->b_off.as<long long>(), c->b_cnt.as<int32_t>(),
                           c->b_rid.as<int32_t>(), c->b_s.as<int32_t>(), c->b_e.as<int32_t>());
    }
    P.sb.n_seg = 1; P.sb.start[0] = 0; P.sb.start[1] = cap_iv;
    P.seg_end_dev = c->b_off.as<long long>() + N;   // the true interval count lives at b_off[N]
    pa.iv_rid = c->b_rid.as<int32_t>(); pa.iv_s = c->b_s.as<int32_t>(); pa.iv_e = c->b_e.as<int32_t>(); pa.n_seg = 1;
    if (P.bwin) {                                   // (the kernel takes its records' reads from the offsets: pileup_wave.hpp IN = 1)
        pa.iv_w = c->b_s.as<uint32_t>();
        pa.grp.off = c->b_off.as<long long>(); pa.grp.stride = N + 1;
        for (int s2 = 0; s2 < kMaxSeg; ++s2) pa.grp.adj[s2] = 0;
    }
    c->sum.interval_path = 1; c->sum.n_segments = P.n_desc + 1; c->sum.n_intervals = -1; // read back in finish
    // (an assignment but for the quantum's bit: a pass that comes here was neither speculated nor did it keep its geometry)
    c->sum.flags = (c->sum.flags & RAFT_HIP_SUM_GRADED_RANGES) | (P.bwin ? RAFT_HIP_SUM_BUCKET_WINDOWS : 0);
    return RAFT_HIP_OK;
}

// The intervals the pileup kernel reads: the caller's columns by the caller's offsets (grouped), the columns as a handful of
// sorted runs (fast), or every side bucketed by read first.
static int interval_source(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &in, PassPlan &P, PileupArgs &pa)
{
    if (P.n_rec == 0) {
        pa.n_seg = 0;
        c->sum.interval_path = 0; c->sum.n_segments = 0; c->sum.n_intervals = 0;
    } else if (P.grouped) {
        P.sb.n_seg = P.eff_runs;                          // (where the runs begin is in the offsets, on the device)
        pa.iv_rid = P.d_qid; pa.iv_s = P.d_qs; pa.iv_e = P.d_qe; pa.n_seg = P.sb.n_seg;
        pa.iv_w = P.lean ? P.d_win : nullptr; pa.grp = P.grp;
        c->sum.interval_path = 0; c->sum.n_segments = in.n_runs; c->sum.n_intervals = P.n_rec;   // (more than kMaxSeg runs: merged into one first)
    } else if (P.fast) {
        std::sort(P.desc, P.desc + P.n_desc);
        P.sb.n_seg = P.n_desc + 1;
        P.sb.start[0] = 0;
        for (int i = 0; i < P.n_desc; ++i) P.sb.start[i + 1] = P.desc[i];
        P.sb.start[P.n_desc + 1] = P.n_rec;
        pa.iv_rid = P.d_qid; pa.iv_s = P.d_qs; pa.iv_e = P.d_qe; pa.n_seg = P.sb.n_seg;
        c->sum.interval_path = 0; c->sum.n_segments = P.sb.n_seg; c->sum.n_intervals = P.n_rec;
    } else
        return bucket_sides(c, P, pa);
    return RAFT_HIP_OK;
}

// The boundaries, the dominant kernel between ev_pile0 and ev_pile1, and what follows it: the deep tiles, delta4's listed windows.
static int launch_pileup(raft_hip_ctx *c, PassPlan &P, PileupArgs &pa)
{
    hipStream_t st = P.st;
    Ctrl *ctrl = P.ctrl;
    const int ow = P.ow;
    // the detection of a pass that assumes a symmetric PAF: one more boundary search of this kernel (pileup.hpp MirrorArgs)
    MirrorArgs mir{};
    if (P.spec && c->prm.symmetric_mode < 0 && P.fast) mir = {P.d_qs, P.d_qe, P.d_tid, P.d_ts, P.d_te, &ctrl->insp.sym_found};
    hipLaunchKernelGGL(tile_desc_kernel, dim3((unsigned)((P.n_tiles + 2 + 255) / 256)), dim3(256), 0, st, P.n_tiles, P.sb, P.seg_end_dev,
                       pa.iv_rid, c->tile_first.as<int32_t>(), c->cov_off.as<long long>(), c->tile_cuts.as<TileCut>(),
                       (P.fast && P.table_ok) ? c->samples.as<int32_t>() : nullptr, (long long)P.n_rec,
                       c->sum.interval_path == 1 ? c->b_off.as<long long>() : nullptr, &ctrl->err_flags, mir, P.grp,
                       P.speculate ? &ctrl->guess : nullptr);
    // ---- the dominant kernel: ONE launch of a persistent grid of single-wave workers, each drawing ranges of reads from the
    // boundaries tile_desc_kernel cut (workers without a range leave at once)
    hc_mark(P, "tile_desc launched");
    HIP_TRY(c, hipEventRecord(c->ev_pile0, st));
    hc_mark(P, "ev_pile0");
    const bool win = P.lean || P.bwin;
    int n_waves = (int)std::max<long long>(1, std::min<long long>(wave_grid_waves(win), P.n_tiles));
    pa.tile_batch = (pa.tile_batch & kCovLineBit) | 1;
    int n_ctr = 8;
#ifdef RAFT_WAVE_DIAG   // (make DEFS=-DRAFT_WAVE_DIAG: run-time switches for tools/mode_probe.py -- workers, parts of the kernel, counters)
    if (const char *e = getenv("RAFT_WAVE_WAVES")) n_waves = std::max(1, std::min(n_waves, atoi(e)));
    if (const char *e = getenv("RAFT_WAVE_MODE")) pa.tile_batch |= std::min(15, std::max(0, atoi(e))) << 20;
    if (const char *e = getenv("RAFT_WAVE_COUNTERS")) n_ctr = std::min(kWaveCounters, std::max(1, atoi(e)));
#endif
    pa.tile_batch |= (n_ctr - 1) << 24;
    pa.piece_w = (int32_t)std::min<long long>(P.extra_cap, INT32_MAX);    // (delta4: tile ids below this have slots of their own)
    launch_wave_variant(ow, win, st, pa.n_seg, c->tile_cuts.p, &pa, n_waves);
    P.n_waves = n_waves;
    // where the coverage array lies, decided by measurement: opt-in, once per capacity of the array (engine_placement.hip)
    if (ow == 4 && c->cov.cap >= DevBuf::kSpreadMin && c->cov.va_bytes && c->cov_trial_cap != c->cov.cap && !c->is_lane && c->trial_candidates > 1 &&
        !DevBuf::policy_explicit().load())
        PHASE(placement_trial(c, st, pa, ow, win, n_waves, P.N));
    hc_mark(P, "pileup launched");
    HIP_TRY(c, hipEventRecord(c->ev_pile1, st));
    // the tiles the wave kernel listed instead of piling them up (2^15 intervals or more: pileup_deep.hpp); nearly always none
    if (!c->deep_skipped)
        hipLaunchKernelGGL(pileup_deep_kernel, dim3(1024), dim3(kDeepThreads), 0, st, pa, c->deep_list.as<DeepTile>(), &ctrl->n_deep, pa.deep_cap, ow);
    hc_mark(P, "ev_pile1");
    if (ow == kCovDelta4)      // the windows the tiles listed, gathered into the shared list (whose counter the control block carries)
        hipLaunchKernelGGL(compact_exceptions_kernel, dim3((unsigned)((P.d4_tiles + kCompactTiles - 1) / kCompactTiles)), dim3(256), 0, st, P.d4_tiles, kExcPerTile,
                           c->exc_tile_n.as<int32_t>(), c->exc_pidx.as<long long>(), c->exc_pval.as<int32_t>(), &ctrl->n_exc, c->exc_cap, c->exc_idx.as<long long>(), c->exc_val.as<int32_t>());
    return RAFT_HIP_OK;
}

// ---- per-read tail: order repeats, mask markers, fragments; the control block handed over; the pass's last event
static int launch_tail(raft_hip_ctx *c, PassPlan &P)
{
    hipStream_t st = P.st;
    Ctrl *ctrl = P.ctrl;
    long long *const tail_part = c->tail_buf.as<long long>(), *const tail_prefix = tail_part + (size_t)4 * P.tail_blocks;
    FinalizeArgs fa{};
    fa.n_reads = P.n_reads; fa.read_len = P.d_len; fa.rep_res_off = c->rep_res_off.as<long long>();
    fa.rep_cnt = c->rep_cnt.as<int32_t>(); fa.raw_key = c->raw_key.as<int32_t>(); fa.raw_s = c->raw_s.as<int32_t>();
    fa.raw_e = c->raw_e.as<int32_t>(); fa.interval_length = c->prm.interval_length; fa.div = c->div;
    fa.overlap_length = c->prm.overlap_length; fa.cut_cnt = c->cut_cnt.as<int32_t>(); fa.frag_cnt = c->frag_cnt.as<int32_t>();
    fa.rep_off = c->rep_off.as<long long>(); fa.cut_off = c->cut_off.as<long long>(); fa.frag_off = c->frag_off.as<long long>();
    fa.rep_s = c->rep_s.as<int32_t>(); fa.rep_e = c->rep_e.as<int32_t>(); fa.cuts = c->cuts.as<int32_t>();
    fa.frag_read = c->frag_read.as<int32_t>(); fa.frag_begin = c->frag_begin.as<int32_t>(); fa.frag_end = c->frag_end.as<int32_t>();
    fa.err_flags = &ctrl->err_flags; fa.err_index = &ctrl->err_index;
    fa.by_L = make_fast_div(c->prm.interval_length); fa.by_div = make_fast_div(c->div); fa.by_reso = make_fast_div(c->prm.reso);
    fa.long_windows = kTileCap; fa.reso = c->prm.reso; fa.repeat_length = c->prm.repeat_length;
    fa.flank = c->prm.flanking_length; fa.rep_cnt_rw = c->rep_cnt.as<int32_t>(); fa.total_repeat = &ctrl->totals[1];
    fa.tail_part = tail_part; fa.tail_prefix = tail_prefix; fa.tail_blocks = P.tail_blocks;
    fa.rep_off_w = c->rep_off.as<long long>(); fa.cut_off_w = c->cut_off.as<long long>(); fa.frag_off_w = c->frag_off.as<long long>();
    // The tail: count -> prefix -> fill -> publish (finalize.hpp FinalizeArgs::tail_part).  The fill kernel makes the three offset
    // arrays on its way; one workgroup in between turns the count kernel's per-workgroup sums into bases and into the totals the
    // host is handed; the last kernel, one wave, hands the control block over -- one block (+1024 bytes) of the context's
    // page-locked memory, stamped with the pass's number.
    const unsigned rgrid = (unsigned)P.tail_blocks;
    TailPublish tp{};
    tp.n_tiles = (long long)P.n_waves; tp.tile_sums = c->block_sums.as<long long>(); tp.totals = ctrl->totals;
    tp.bucket_off = c->sum.interval_path == 1 ? c->b_off.as<long long>() : nullptr; tp.tails = ctrl->out_totals;
    tp.ctrl_words = reinterpret_cast<const long long *>(ctrl); tp.n_ctrl_words = (int)(sizeof(Ctrl) / 8);
    tp.host_block = c->pinned_dev + 128; tp.pass_seq = ++c->pass_seq;
    if (P.N > 0) hipLaunchKernelGGL(finalize_count_kernel, dim3(rgrid), dim3(256), 0, st, fa);
    hipLaunchKernelGGL(tail_prefix_kernel, dim3((unsigned)((P.tail_blocks + 1023) / 1024)), dim3(1024), 0, st, fa, tp);
    if (P.N > 0) {
        if (c->emit_cuts) hipLaunchKernelGGL(finalize_fill_kernel<true>, dim3(rgrid), dim3(256), 0, st, fa);
        else hipLaunchKernelGGL(finalize_fill_kernel<false>, dim3(rgrid), dim3(256), 0, st, fa);
    }
    hipLaunchKernelGGL(publish_and_clear_kernel, dim3(1), dim3(64), 0, st, tp, reinterpret_cast<long long *>(ctrl), c->wave_ctr.as<int32_t>(),
                       (int)(offsetof(Ctrl, err_index) / 8), (int)((offsetof(Ctrl, insp) + offsetof(InspectOut, err_index)) / 8));
    c->seq_armed = true;
    c->ctrl_clean = true; c->clean_stream = st;
    c->fa = fa; c->cuts_ready = c->emit_cuts;
    c->pass_width = P.ow; c->cov_valid = P.ow == 4;
    hc_mark(P, "tail launched");
    HIP_TRY(c, hipEventRecord(c->ev_pass1, st));
    HIP_TRY(c, hipGetLastError());
    hc_mark(P, "ev_pass1");
    return RAFT_HIP_OK;
}

// One pass.  `verify_in_kernels` (the default): no full look at the record
// stream at all (inspect_kernel: ids in range, sorted runs -- one read of the qid column, 0.22-0.24 ms at human scale,
// all of it ahead of the pass's host wait).  A one-workgroup-per-CU kernel samples the stream and names the sorted runs;
// the pass is built on that, and what makes it safe is that tile_desc_kernel and the pileup kernels enforce what they
// rely on: tile ranges tile every run exactly, and every record is checked against the reads of the tile (sub-batch,
// chunk) that processes it.  A record that refutes the guess -- an id out of range, a dip in the order between two
// samples -- raises kErrOrder, and raft_hip_finish() then runs the pass again from the same arguments, this time after
// inspect_kernel has looked at every record (which also reports errors exactly as before).  A detecting context
// (symmetric_mode = -1) assumes the symmetric PAF hifiasm writes and has tile_desc_kernel search for the mirror of
// record 0 where sorted runs keep it (among the records of record 0's target: pileup.hpp MirrorArgs); none found sends
// the pass to the second form too, and the context then stops assuming until a pass of its own detects a symmetric PAF.
// (Measured and dropped: starting on the guess and running inspect_kernel BESIDE the pileup kernels on a low-priority
// stream -- it costs the pileup what it would cost alone, 0.15-0.2 ms; the pass did not get shorter.)
//
// The grouped form (raft_hip_run_device_grouped; `in.rec_off`): the caller says where every read's records begin in every
// run, so nothing is guessed or searched -- the runs are what the offsets say, tile cuts are look-ups -- and, as in a
// verified pass, every record is still checked against the reads of the tile that processes it (with a query column
// at hand; without one the ids ARE the offsets, expanded on the device).  A record that does not sit where the offsets
// say sends the pass to the plain form above.  With the caller's window count (`in.hint_bins`) the host sizes everything
// without waiting for the device: the pass is one uninterrupted sequence of launches.
//
// The forms of a pass, by what the phases below do for them:
//   plain with host wait      side-stream scan beside guess / inspect, sizes read back, tile_first_kernel
//   speculated                sizes and run ends remembered (Shape), fused head, no wait
//   ... with kept geometry    verify_lengths_kernel for a head
//   grouped with hint         sizes from the caller's count, fused head, no wait
//   grouped with host wait    scan on the main stream, sizes read back, tile_first_kernel
// A HIP error or RAFT_HIP_ERR_TOO_LARGE on the way leaves c->ran false; an input error the host sees is parked (park_input_error).
int run_pass(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &in, bool verify_in_kernels)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    SyncScope scope(c->stream, c->side_stream);            // (a buffer that grows waits for this context's streams only)
    PassPlan P{};
    P.sw = read_switches();
    PHASE(resolve_input(c, in, P));
    reset_and_decide(c, in, verify_in_kernels, P);
    PHASE(open_pass(c, in, P));
    PHASE(find_sizes(c, in, P));
    if (P.parked) return RAFT_HIP_OK;
    choose_quantum(c, P);
    PHASE(ensure_buffers(c, P));
    hc_mark(P, "sized");
    launch_head(c, in, P);
    PHASE(decide_source(c, P));
    if (P.look_again) return run_pass(c, in, false);       // (the head is queued; the pass begins again on entry, state reset included)
    if (P.parked) return RAFT_HIP_OK;
    PileupArgs pa{};
    PHASE(fill_pileup_args(c, P, pa));
    PHASE(interval_source(c, in, P, pa));
    PHASE(launch_pileup(c, P, pa));
    PHASE(launch_tail(c, P));
    c->ran = true;
    return RAFT_HIP_OK;
}

int run_grouped(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_len, int64_t n_rec, int32_t n_runs, const int64_t *d_rec_offset,
                const long long *adj, const int32_t *d_qid, const int32_t *d_qs, const int32_t *d_qe, int64_t n_bins,
                const uint32_t *d_win)
{
    if (!c || !d_rec_offset) return RAFT_HIP_ERR_PARAM;
    if (n_rec > 0 && !d_win && (!d_qs || !d_qe)) {          // (what an exchange of window records hands back goes to raft_hip_run_device_windows)
        c->last_error = "grouped input: records without both coordinate columns";
        return RAFT_HIP_ERR_PARAM;
    }
    if (c->force_bucket && d_qid && c->prm.symmetric_mode == 1)          // (tests, A/B: the counting-sort path needs no offsets)
        return raft_hip_run_device(c, n_reads, d_len, n_rec, d_qid, d_qs, d_qe, nullptr, nullptr, nullptr);
    raft_hip_ctx::PassArgs in{};
    in.n_reads = n_reads; in.len = d_len; in.n_rec = n_rec;
    in.col[0] = d_qid; in.col[1] = d_qs; in.col[2] = d_qe; in.win = d_win;
    in.n_runs = n_runs; in.rec_off = reinterpret_cast<const long long *>(d_rec_offset);
    for (int s = 0; s < kMaxSeg; ++s) in.adj[s] = adj ? adj[s] : 0;
    in.hint_bins = n_bins >= 0 ? n_bins : -1;
    return run_pass(c, in, true);
}

// the control block as the pass's last workgroup handed it over (publish_and_clear_kernel: stamped lines, 1024 bytes into the page-locked block)
Ctrl host_ctrl(const raft_hip_ctx *c)
{
    static_assert(sizeof(Ctrl) % 8 == 0 && sizeof(Ctrl) / 8 <= 48, "the control block travels in one wave's stamped lines");
    long long w[sizeof(Ctrl) / 8];
    unstamp(reinterpret_cast<const volatile long long *>(c->pinned) + 128, (int)(sizeof(Ctrl) / 8), w);
    Ctrl hc;
    memcpy(&hc, w, sizeof(Ctrl));
    return hc;
}

// ---- raft_hip_finish in three parts: wait for the pass, run it again where a kernel objected, collect the summary

// The pass's last workgroup writes the pass's number behind the control block: seen there, everything is done.  The host
// looks for it itself for a while (a pass is 0.2-3 ms: bounded by 4 ms) and falls back to the runtime's wait (wait_stamped).
static int wait_for_pass(raft_hip_ctx *c)
{
    bool seen = false;
    PHASE(wait_stamped(c, reinterpret_cast<const volatile long long *>(c->pinned) + 128, (int)(sizeof(Ctrl) / 8), c->pass_seq, c->seq_armed ? 4 : 0,
                       c->stream, &seen));
    if (seen) {                                          // (the number was seen without the runtime: a fault of this pass still surfaces here)
        const hipError_t q = hipStreamQuery(c->stream);
        if (q != hipSuccess && q != hipErrorNotReady) return fail_hip(c, q, "hipStreamQuery after the pass");
    }
    return RAFT_HIP_OK;
}

// the pass once more, and to its end; !verify_in_kernels: this time nothing assumed
static int run_again(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &a, bool verify_in_kernels, int *n_reruns)
{
    ++*n_reruns;
    PHASE(run_pass(c, a, verify_in_kernels));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!verify_in_kernels) c->spec = false;
    return RAFT_HIP_OK;
}

// What a pass was built on and a kernel refuted: the pass is run again without it.  Five steps, in this order -- each looks at the
// control block of the pass that ran last, which may be the re-run of the step before.
static int rerun_ladder(raft_hip_ctx *c, int *n_reruns)
{
    if (c->speculated && c->pending_err == RAFT_HIP_OK) {
        const Ctrl hc = host_ctrl(c);
        if (hc.err_flags & kErrHint) {
            // the stream is not what the context's last pass saw (other lengths, other run ends): the pass again, nothing remembered
            c->shape.valid = false;
            PHASE(run_again(c, c->args, true, n_reruns));
        }
    }
    if (c->grouped && c->pending_err == RAFT_HIP_OK) {
        const Ctrl hc = host_ctrl(c);
        if (hc.err_flags & kErrHint) {
            // the caller's window count is not what the read lengths give: the same pass, sized by the device's own count
            auto a = c->args;
            a.hint_bins = -1;
            PHASE(run_again(c, a, false, n_reruns));
        }
    }
    if (c->grouped && c->pending_err == RAFT_HIP_OK) {
        const Ctrl hc = host_ctrl(c);
        if ((hc.err_flags & (kErrOrder | kErrReadId)) && !(hc.err_flags & kErrStop) && c->args.col[0]) {
            // a record does not sit where the caller's offsets say: the offsets are dropped and the query column is
            // taken for what it is (the plain pass, after a look at every record)
            auto a = c->args;
            a.rec_off = nullptr; a.n_runs = 0; a.hint_bins = -1;
            PHASE(run_again(c, a, false, n_reruns));
        }
    }
    if (c->spec && c->pending_err == RAFT_HIP_OK) {
        // did a kernel meet a record that refutes the sampled guess the pass was built on?
        const Ctrl hc = host_ctrl(c);
        c->spec = false;
        const bool no_mirror = c->prm.symmetric_mode < 0 && hc.insp.sym_found == 0;   // assumed symmetric, found no mirror
        if (no_mirror) c->assume_sym = false;
        if ((hc.err_flags & (kErrOrder | kErrReadId)) || no_mirror) {   // run it again, this time after looking at every record
            c->shape.valid = false;
            PHASE(run_again(c, c->args, false, n_reruns));
        }
    }
    // Three more reasons to run the pass again, each of which may turn up in the re-run of another:
    //  * kErrWide: general bucketing, a side whose windows do not fit 16 bits -> coordinate pairs from now on;
    //  * kErrDeep: more tiles of 2^15 intervals or more than the list for pileup_deep_kernel held -> once more, with room;
    //  * more windows at or above the encoding's limit than the list held -> once more with room for all of them.
    for (int round = 0; round < 4 && c->pending_err == RAFT_HIP_OK; ++round) {
        const Ctrl hc = host_ctrl(c);
        if (hc.err_flags & kErrStop) break;
        bool rerun = false;
        if ((hc.err_flags & kErrWide) && !c->no_bucket_win) {
            c->no_bucket_win = true;            // a side's windows do not fit 16 bits: this context buckets coordinate pairs from now on
            rerun = true;
        } else if ((hc.err_flags & kErrDeep) && ((long long)hc.n_deep > c->deep_cap || c->deep_skipped)) {
            // more deep tiles than the list held -- or a pass that was launched without the side kernel met one: once more, with room
            c->deep_cap = std::max(c->deep_cap, (long long)hc.n_deep + 64);
            c->shape.had_deep = true;
            rerun = true;
        } else if (c->pass_width != 4 && (long long)hc.n_exc > c->exc_cap && !(hc.err_flags & ~(kErrOrder | kErrDeep | kErrWide))) {
            c->exc_cap = (long long)hc.n_exc;
            rerun = true;
        }
        if (!rerun) break;
        PHASE(run_again(c, c->args, false, n_reruns));
    }
    return RAFT_HIP_OK;
}

// what the pass that stands reports: counts and totals from the control block it handed over, its error if it met one
static void collect_summary(raft_hip_ctx *c, int n_reruns)
{
    if (c->pending_err == RAFT_HIP_OK) {
        const Ctrl hc = host_ctrl(c);   // copied at the end of the pass
        if (c->pass_width != 4) { c->n_exc = (long long)hc.n_exc; c->packed_width = c->pass_width; c->exc_sorted = false; }
        c->sum.n_repeats = hc.out_totals[0]; c->sum.n_cuts = hc.out_totals[1]; c->sum.n_fragments = hc.out_totals[2];
        if (c->sum.interval_path == 1) c->sum.n_intervals = hc.out_totals[3];
        c->sum.total_coverage = (long long)hc.totals[0];
        c->sum.total_repeat_length = (long long)hc.totals[1];
        c->sum.total_read_length = (long long)hc.totals[2];
        if (hc.n_deep > 0) c->sum.flags |= RAFT_HIP_SUM_DEEP_TILES;
        c->shape.had_deep = hc.n_deep > 0;
        if (hc.err_flags) {
            c->pending_err = code_from_flags(hc.err_flags);
            c->pending_err_index = hc.err_index;
        }
        // a speculative pass that scanned the geometry afresh and came through clean: the passes after it may keep it
        if (c->spec_scanned && n_reruns == 0 && !hc.err_flags && c->shape.valid && c->geom_id == c->spec_geom_id)
            c->shape.geom_id = c->geom_id;
    }
    if (n_reruns > 0) c->sum.flags |= RAFT_HIP_SUM_RERUN;
    c->sum.error_index = c->pending_err ? c->pending_err_index : -1;
}

// The cut points (one int per kept marker, 0.4 GB at human scale) are not written by the pass: the fragments are
// derived while the markers are walked.  The first caller that asks for them pays for one more per-read kernel.
static int materialise_cuts(raft_hip_ctx *c)
{
    if (c->cuts_ready) return RAFT_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->sum.n_reads > 0) {
        hipLaunchKernelGGL(finalize_cuts_kernel, dim3((unsigned)((c->sum.n_reads + 255) / 256)), dim3(256), 0, c->stream, c->fa);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->cuts_ready = true;
    return RAFT_HIP_OK;
}

// cov[] as int32 after a pass that wrote its encoding directly: decoded on the device, once, for the caller that asks.  (Without
// the int32 array the pass wrote one or two bytes a window or four-bit steps: decode_cov's answer for any other width cannot come.)
static int materialise_cov(raft_hip_ctx *c)
{
    if (c->cov_valid) return RAFT_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(decode_cov(c, c->cov, c->abs_bits, "materialise_cov"));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->cov_valid = true;
    return RAFT_HIP_OK;
}

static int queue_repeat_rows(raft_hip_ctx *c, int64_t *rep_offset, int32_t *rep_s, int32_t *rep_e)
{
    return queue_copies(c, {{rep_offset, c->rep_off.p, ((size_t)c->sum.n_reads + 1) * 8}, {rep_s, c->rep_s.p, (size_t)c->sum.n_repeats * 4},
                            {rep_e, c->rep_e.p, (size_t)c->sum.n_repeats * 4}});
}
static int queue_fragment_rows(raft_hip_ctx *c, int64_t *frag_offset, int32_t *frag_read, int32_t *frag_begin, int32_t *frag_end)
{
    return queue_copies(c, {{frag_offset, c->frag_off.p, ((size_t)c->sum.n_reads + 1) * 8}, {frag_read, c->frag_read.p, (size_t)c->sum.n_fragments * 4},
                            {frag_begin, c->frag_begin.p, (size_t)c->sum.n_fragments * 4}, {frag_end, c->frag_end.p, (size_t)c->sum.n_fragments * 4}});
}

// cov[] -> one or two bytes per window + exception list (pack.hpp), on the device, once per pass and width
int pack_coverage(raft_hip_ctx *c, int width)
{
    if (c->packed_width == width) return RAFT_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(materialise_cov(c));                             // (a pass that wrote the other width)
    const long long B = c->sum.n_bins;
    const bool d4 = width == kCovDelta4;
    HIP_TRY(c, c->cov8.ensure(d4 ? (size_t)std::max(B, 1LL) / 2 + 16 : (size_t)std::max(B, 1LL) * (size_t)width + 16));
    if (d4) HIP_TRY(c, c->cov_anchor.ensure(((size_t)std::max(B, 1LL) / kD4Block + 3) * 4));
    HIP_TRY(c, c->exc_cnt.ensure(8));
    long long cap = std::max<long long>(c->exc_cap, std::max<long long>(4096, d4 ? B / 64 : B / 512));
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIP_TRY(c, c->exc_idx.ensure((size_t)cap * 8));
        HIP_TRY(c, c->exc_val.ensure((size_t)cap * 4));
        c->exc_cap = cap;
        HIP_TRY(c, hipMemsetAsync(c->exc_cnt.p, 0, 8, c->stream));
        if (B > 0) {
            const unsigned grid = grid_for(B / 4, 1024, 256 * 16);
            if (d4) {
                Delta4Out po{c->cov8.as<uint8_t>(), c->cov_anchor.as<int32_t>(), c->exc_cnt.as<unsigned long long>(), cap, c->exc_idx.as<long long>(), c->exc_val.as<int32_t>()};
                hipLaunchKernelGGL(pack_delta4_kernel, dim3(grid), dim3(256), 0, c->stream, c->cov.as<int32_t>(), B, po, c->d4_shift);
            } else if (width == 1) {
                PackOut<uint8_t> po{c->cov8.as<uint8_t>(), c->exc_cnt.as<unsigned long long>(), cap, c->exc_idx.as<long long>(), c->exc_val.as<int32_t>()};
                hipLaunchKernelGGL(pack_cov_kernel<uint8_t>, dim3(grid), dim3(256), 0, c->stream, c->cov.as<int32_t>(), B, po);
            } else {
                PackOut<uint16_t> po{c->cov8.as<uint16_t>(), c->exc_cnt.as<unsigned long long>(), cap, c->exc_idx.as<long long>(), c->exc_val.as<int32_t>()};
                hipLaunchKernelGGL(pack_cov_kernel<uint16_t>, dim3(grid), dim3(256), 0, c->stream, c->cov.as<int32_t>(), B, po);
            }
            HIP_TRY(c, hipGetLastError());
        }
        long long *h = reinterpret_cast<long long *>(c->pinned) + kPackCountWord;
        HIP_TRY(c, hipMemcpyAsync(h, c->exc_cnt.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->n_exc = *h; c->exc_sorted = false;
        if (c->n_exc <= cap) break;
        cap = c->n_exc;                              // (rare) more windows at or above the limit than the list held: once more
    }
    c->packed_width = width;
    return RAFT_HIP_OK;
}

// The kernels append exceptions in no particular order; callers get them ascending by window.  With a byte per window there
// are none on a 32x set; the four-bit encoding lists 0.2-0.3 % of the windows (3.7e6 at human scale) and the host's
// std::sort of a chunk's 3.4e5 pairs held its lane for 25 ms: sorted on the device (radix sort on the index bits in use).
int sort_exceptions(raft_hip_ctx *c)
{
    if (c->exc_sorted || c->n_exc < 2) { c->exc_sorted = true; return RAFT_HIP_OK; }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->n_exc;
    HIP_TRY(c, c->exc_idx2.ensure(std::max(n * 8, c->exc_idx.cap)));
    HIP_TRY(c, c->exc_val2.ensure(std::max(n * 4, c->exc_val.cap)));
    int bits = 1;
    while (bits < 63 && (1LL << bits) <= std::max<long long>(c->sum.n_bins, 1)) ++bits;
    using Key = unsigned long long;           // (window indices are non-negative)
    HIP_TRY(c, c->sort_tmp.ensure(sort_pairs_hist_bytes((long long)n)));
    bool in_b = false;
    HIP_TRY(c, sort_pairs(c->stream, c->exc_idx.as<Key>(), c->exc_val.as<int32_t>(), c->exc_idx2.as<Key>(), c->exc_val2.as<int32_t>(), (long long)n, bits,
                          c->sort_tmp.as<int32_t>(), &in_b));
    if (in_b) { std::swap(c->exc_idx, c->exc_idx2); std::swap(c->exc_val, c->exc_val2); }
    c->exc_sorted = true;
    return RAFT_HIP_OK;
}

int fetch_packed_impl(raft_hip_ctx *c, int32_t width, int64_t *cov_offset, void *cov_packed, int32_t *cov_anchor, int64_t exc_cap, int64_t *exc_index,
                      int32_t *exc_value, int64_t *n_exc, int64_t *rep_offset, int32_t *rep_s, int32_t *rep_e,
                      int64_t *frag_offset, int32_t *frag_read, int32_t *frag_begin, int32_t *frag_end)
{
    if (!c || !n_exc || (width != 1 && width != 2 && width != kCovDelta4)) return RAFT_HIP_ERR_PARAM;
    if (!c->finished || c->pending_err) return RAFT_HIP_ERR_STATE;
    { const int rc = pack_coverage(c, width); if (rc != RAFT_HIP_OK) return rc; }
    *n_exc = c->n_exc;
    // (*n_exc tells the caller what to provide; the size query -- every pointer NULL -- always succeeds)
    if (c->n_exc > exc_cap && (cov_packed || exc_index || exc_value)) return RAFT_HIP_ERR_TOO_LARGE;
    if (exc_index || exc_value) { const int rc = sort_exceptions(c); if (rc != RAFT_HIP_OK) return rc; }   // handed out ascending by window
    const bool d4 = width == kCovDelta4;
    PHASE(queue_copies(c, {{cov_packed, c->cov8.p, d4 ? ((size_t)c->sum.n_bins + 1) / 2 : (size_t)c->sum.n_bins * (size_t)width},
                           {cov_offset, c->cov_off.p, ((size_t)c->sum.n_reads + 1) * 8},
                           {d4 ? cov_anchor : nullptr, c->cov_anchor.p, (((size_t)c->sum.n_bins + kD4Block - 1) / kD4Block) * 4},
                           {exc_index, c->exc_idx.p, (size_t)c->n_exc * 8}, {exc_value, c->exc_val.p, (size_t)c->n_exc * 4}}));
    PHASE(queue_repeat_rows(c, rep_offset, rep_s, rep_e));
    PHASE(queue_fragment_rows(c, frag_offset, frag_read, frag_begin, frag_end));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RAFT_HIP_OK;
}

} // namespace raft

extern "C" {

int raft_hip_abi_version(void) { return RAFT_HIP_ABI_VERSION; }

const char *raft_hip_strerror(int code)
{
    switch (code) {
    case RAFT_HIP_OK: return "ok";
    case RAFT_HIP_ERR_PARAM: return "invalid parameter (reso/est_cov/repeat_length/interval_length <= 0, read_length < interval_length, or negative read length)";
    case RAFT_HIP_ERR_READ_ID: return "PAF record names a read id outside [0, n_reads)";
    case RAFT_HIP_ERR_COORD: return "PAF coordinate negative or beyond the last coverage window of its read";
    case RAFT_HIP_ERR_FRAGMENT: return "fragment would start before base 0 (overlap_length larger than its first cut point)";
    case RAFT_HIP_ERR_NOMEM: return "out of memory";
    case RAFT_HIP_ERR_DEVICE: return "HIP device/runtime error";
    case RAFT_HIP_ERR_STATE: return "call order violated";
    case RAFT_HIP_ERR_TOO_LARGE: return "input too large for 32-bit per-read quantities";
    default: return "unknown error";
    }
}

const char *raft_hip_last_error(const raft_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

// A context's events: what they are made with (hipEventDefault: they time) and whether at raft_hip_create or by their first user.
// raft_hip_destroy destroys the ones that exist.
struct CtxEvent { hipEvent_t raft_hip_ctx::*ev; unsigned flags; bool on_demand; };
static const CtxEvent kCtxEvents[] = {
    {&raft_hip_ctx::ev_ifork, hipEventDisableTiming, false}, {&raft_hip_ctx::ev_gjoin, hipEventDisableTiming, false},
    {&raft_hip_ctx::ev_pass0, hipEventDefault, false},       {&raft_hip_ctx::ev_pass1, hipEventDefault, false},
    {&raft_hip_ctx::ev_pile0, hipEventDefault, false},       {&raft_hip_ctx::ev_pile1, hipEventDefault, false},
    {&raft_hip_ctx::ev_hist0, hipEventDefault, true},        {&raft_hip_ctx::ev_hist1, hipEventDefault, true}};

int raft_hip_create(int device_id, const raft_hip_params *params, raft_hip_ctx **out)
{
    if (!out) return RAFT_HIP_ERR_PARAM;
    *out = nullptr;
    int rc = check_params(params);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return RAFT_HIP_ERR_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return RAFT_HIP_ERR_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RAFT_HIP_ERR_DEVICE; // kernels are built for gfx950 only
    raft_hip_ctx *c = new (std::nothrow) raft_hip_ctx();
    if (!c) return RAFT_HIP_ERR_NOMEM;
    c->device = device_id;
    apply_params(c, params);
    if (const char *w = getenv("RAFT_COV_WIDTH")) {           // (test sweeps: every context of the process in that width)
        const int v = atoi(w);
        if (v == 1 || v == 2 || v == 4 || v == kCovDelta4) c->out_width = v;
    }
    bool ok = hipSetDevice(device_id) == hipSuccess && hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) == hipSuccess &&
              hipHostMalloc(&c->pinned, 4096, hipHostMallocDefault) == hipSuccess &&
              hipHostGetDevicePointer(reinterpret_cast<void **>(&c->pinned_dev), c->pinned, 0) == hipSuccess;
    for (const CtxEvent &e : kCtxEvents)
        if (ok && !e.on_demand) ok = hipEventCreateWithFlags(&(c->*e.ev), e.flags) == hipSuccess;
    if (!ok) {
        raft_hip_destroy(c);
        return RAFT_HIP_ERR_DEVICE;
    }
    c->stream = c->own_stream;
    memset(c->pinned, 0, 4096);                            // (the pass numbers raft_hip_finish looks for start at 1)
    { ChunkPool &pool = ChunkPool::of(device_id); std::lock_guard<std::mutex> lk(pool.mu); ++pool.live_ctx; }
    c->counted = true;
    *out = c;
    return RAFT_HIP_OK;
}

void raft_hip_destroy(raft_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (raft_hip_ctx *l : c->lanes) raft_hip_destroy(l);
    if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
    if (c->down_stream) (void)hipStreamSynchronize(c->down_stream);
    SyncScope scope(c->stream, c->side_stream);            // (the buffers' releases wait for this context's streams, not the device)
    c->lanes.clear();
    for (hipEvent_t e : c->lane_up_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->lane_down_ev) (void)hipEventDestroy(e);
    c->lane_up_ev.clear(); c->lane_down_ev.clear();
    if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
    if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
    for (DevBuf *b : c->bufs) b->release();
    for (DevBuf *b : c->user_bufs) { b->release(); delete b; }
    c->user_bufs.clear();
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (const CtxEvent &e : kCtxEvents)
        if (c->*e.ev) (void)hipEventDestroy(c->*e.ev);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->counted) {                                      // the device's last context hands the pooled chunks back to the driver
        ChunkPool &pool = ChunkPool::of(c->device);
        bool last = false;
        { std::lock_guard<std::mutex> lk(pool.mu); last = --pool.live_ctx == 0; }
        if (last && getenv("RAFT_VMM_KEEP_POOL") == nullptr) (void)pool.trim(0);
    }
    delete c;
}

int raft_hip_set_params(raft_hip_ctx *c, const raft_hip_params *params)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    int rc = check_params(params);
    if (rc) return rc;
    apply_params(c, params);
    return RAFT_HIP_OK;
}

int raft_hip_set_stream(raft_hip_ctx *c, void *stream)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    c->stream = (hipStream_t)stream;
    return RAFT_HIP_OK;
}

int raft_hip_use_own_stream(raft_hip_ctx *c)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    c->stream = c->own_stream;
    return RAFT_HIP_OK;
}

void *raft_hip_get_stream(raft_hip_ctx *c) { return c ? (void *)c->stream : nullptr; }

int raft_hip_set_tuning(raft_hip_ctx *c, int32_t tile_bins, int32_t force_bucket_path, int32_t variant)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    // (variant: rounds 1-5 kept several pileup kernels; -1 and 5 name the one there is -- pileup_wave.hpp -- and nothing else is accepted)
    if (variant != -1 && variant != 5) return RAFT_HIP_ERR_PARAM;
    if (tile_bins < 0 || tile_bins > (1 << 20)) return RAFT_HIP_ERR_PARAM;   // (the quantum is a worker's share of windows per draw, not a tile)
    c->tile_q = tile_bins;
    c->force_bucket = force_bucket_path ? 1 : 0;
    return RAFT_HIP_OK;
}

int raft_hip_run_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_len, int64_t n_rec,
                        const int32_t *d_qid, const int32_t *d_qs, const int32_t *d_qe,
                        const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te)
{
    raft_hip_ctx::PassArgs in{};
    in.n_reads = n_reads; in.len = d_len; in.n_rec = n_rec;
    in.col[0] = d_qid; in.col[1] = d_qs; in.col[2] = d_qe; in.col[3] = d_tid; in.col[4] = d_ts; in.col[5] = d_te;
    in.hint_bins = -1;
    return run_pass(c, in, true);
}

int raft_hip_run_device_grouped(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_len, int64_t n_rec, int32_t n_runs,
                                const int64_t *d_rec_offset, const int32_t *d_qid, const int32_t *d_qs, const int32_t *d_qe,
                                int64_t n_bins)
{
    return run_grouped(c, n_reads, d_len, n_rec, n_runs, d_rec_offset, nullptr, d_qid, d_qs, d_qe, n_bins);
}

int raft_hip_run_device_windows(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_len, int64_t n_rec, int32_t n_runs,
                                const int64_t *d_rec_offset, const uint32_t *d_win, int64_t n_bins)
{
    if (n_rec > 0 && !d_win) return RAFT_HIP_ERR_PARAM;
    static const uint32_t none = 0;                       // (no records: the column is never read, but says which form this is)
    return run_grouped(c, n_reads, d_len, n_rec, n_runs, d_rec_offset, nullptr, nullptr, nullptr, nullptr, n_bins, d_win ? d_win : &none);
}

int raft_hip_run_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec,
                      const int32_t *qid, const int32_t *qs, const int32_t *qe,
                      const int32_t *tid, const int32_t *ts, const int32_t *te)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (n_reads < 0 || n_rec < 0) return RAFT_HIP_ERR_PARAM;
    if (n_reads > 0 && !read_len) return RAFT_HIP_ERR_PARAM;
    // With symmetric_mode = 1 (the tokeniser saw the mirror of record 0, chop.hpp:175-184) only the query side is piled
    // up: the three target columns are neither needed nor uploaded (half of the H2D bytes) and may be NULL.
    const int n_cols = c->prm.symmetric_mode == 1 ? 3 : 6;
    if (n_rec > 0 && (!qid || !qs || !qe || (n_cols == 6 && (!tid || !ts || !te)))) return RAFT_HIP_ERR_PARAM;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->in_len.ensure((size_t)std::max<long long>(n_reads, 1) * 4));
    if (n_reads) HIP_TRY(c, hipMemcpyAsync(c->in_len.p, read_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, st));
    const int32_t *src[6] = {qid, qs, qe, tid, ts, te};
    for (int k = 0; k < n_cols; ++k) {
        HIP_TRY(c, c->in_col[k].ensure((size_t)std::max<long long>(n_rec, 1) * 4));
        if (n_rec) HIP_TRY(c, hipMemcpyAsync(c->in_col[k].p, src[k], (size_t)n_rec * 4, hipMemcpyHostToDevice, st));
    }
    const bool six = n_cols == 6;
    return raft_hip_run_device(c, n_reads, c->in_len.as<int32_t>(), n_rec, c->in_col[0].as<int32_t>(),
                               c->in_col[1].as<int32_t>(), c->in_col[2].as<int32_t>(), six ? c->in_col[3].as<int32_t>() : nullptr,
                               six ? c->in_col[4].as<int32_t>() : nullptr, six ? c->in_col[5].as<int32_t>() : nullptr);
}

int raft_hip_finish(raft_hip_ctx *c, raft_hip_summary *summary)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (!c->ran) return RAFT_HIP_ERR_STATE;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->finished) {
        int n_reruns = 0;
        PHASE(wait_for_pass(c));
        PHASE(rerun_ladder(c, &n_reruns));
        collect_summary(c, n_reruns);
        c->finished = true;
    }
    if (summary) *summary = c->sum;
    return c->pending_err;
}

int raft_hip_set_output_width(raft_hip_ctx *c, int32_t width)
{
    if (!c || (width != 1 && width != 2 && width != 4 && width != kCovDelta4)) return RAFT_HIP_ERR_PARAM;
    c->out_width = width;
    return RAFT_HIP_OK;
}

int raft_hip_set_emit_cuts(raft_hip_ctx *c, int32_t on)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    c->emit_cuts = on != 0;
    return RAFT_HIP_OK;
}

int raft_hip_packed_device(raft_hip_ctx *c, int32_t *width, const void **cov_packed, const int64_t **exc_index,
                           const int32_t **exc_value, int64_t *n_exc)
{
    if (!c || !width) return RAFT_HIP_ERR_PARAM;
    if (!c->finished || c->pending_err) return RAFT_HIP_ERR_STATE;
    *width = c->packed_width;
    const bool have = c->packed_width != 0;
    if (cov_packed) *cov_packed = have ? c->cov8.p : nullptr;
    if (exc_index) *exc_index = have ? c->exc_idx.as<int64_t>() : nullptr;
    if (exc_value) *exc_value = have ? c->exc_val.as<int32_t>() : nullptr;
    if (n_exc) *n_exc = have ? c->n_exc : 0;
    return RAFT_HIP_OK;
}

int raft_hip_packed_anchor_device(raft_hip_ctx *c, const int32_t **cov_anchor, int64_t *n_anchor)
{
    if (!c || !cov_anchor) return RAFT_HIP_ERR_PARAM;
    if (!c->finished || c->pending_err) return RAFT_HIP_ERR_STATE;
    const bool have = c->packed_width == kCovDelta4;
    *cov_anchor = have ? c->cov_anchor.as<int32_t>() : nullptr;
    if (n_anchor) *n_anchor = have ? (c->sum.n_bins + kD4Block - 1) / kD4Block : 0;
    return RAFT_HIP_OK;
}

int raft_hip_outputs_device(raft_hip_ctx *c, raft_hip_outputs *o)
{
    if (!c || !o) return RAFT_HIP_ERR_PARAM;
    if (!c->finished || c->pending_err) return RAFT_HIP_ERR_STATE;
    { const int rc = materialise_cuts(c); if (rc != RAFT_HIP_OK) return rc; }
    PHASE(materialise_cov(c));
    ++c->geom_id;                                  // (cov_offset goes out writable: the next pass scans the geometry again)
    o->cov_offset = c->cov_off.as<int64_t>(); o->cov = c->cov.as<int32_t>();
    o->rep_offset = c->rep_off.as<int64_t>(); o->rep_s = c->rep_s.as<int32_t>(); o->rep_e = c->rep_e.as<int32_t>();
    o->cut_offset = c->cut_off.as<int64_t>(); o->cuts = c->cuts.as<int32_t>();
    o->frag_offset = c->frag_off.as<int64_t>(); o->frag_read = c->frag_read.as<int32_t>();
    o->frag_begin = c->frag_begin.as<int32_t>(); o->frag_end = c->frag_end.as<int32_t>();
    return RAFT_HIP_OK;
}

int raft_hip_fetch(raft_hip_ctx *c, int64_t *cov_offset, int32_t *cov, int64_t *rep_offset, int32_t *rep_s, int32_t *rep_e,
                   int64_t *cut_offset, int32_t *cuts, int64_t *frag_offset, int32_t *frag_read, int32_t *frag_begin,
                   int32_t *frag_end)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (!c->finished || c->pending_err) return RAFT_HIP_ERR_STATE;
    HIP_TRY(c, hipSetDevice(c->device));
    if (cuts) { const int rc = materialise_cuts(c); if (rc != RAFT_HIP_OK) return rc; }
    if (cov) PHASE(materialise_cov(c));
    PHASE(queue_copies(c, {{cov_offset, c->cov_off.p, ((size_t)c->sum.n_reads + 1) * 8}, {cov, c->cov.p, (size_t)c->sum.n_bins * 4}}));
    PHASE(queue_repeat_rows(c, rep_offset, rep_s, rep_e));
    PHASE(queue_copies(c, {{cut_offset, c->cut_off.p, ((size_t)c->sum.n_reads + 1) * 8}, {cuts, c->cuts.p, (size_t)c->sum.n_cuts * 4}}));
    PHASE(queue_fragment_rows(c, frag_offset, frag_read, frag_begin, frag_end));     // (all copies queued on the context's stream, one wait)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RAFT_HIP_OK;
}

int raft_hip_fetch_packed_w(raft_hip_ctx *c, int32_t width, int64_t *cov_offset, void *cov_packed, int64_t exc_cap, int64_t *exc_index,
                            int32_t *exc_value, int64_t *n_exc, int64_t *rep_offset, int32_t *rep_s, int32_t *rep_e,
                            int64_t *frag_offset, int32_t *frag_read, int32_t *frag_begin, int32_t *frag_end)
{
    if (width != 1 && width != 2) return RAFT_HIP_ERR_PARAM;
    return fetch_packed_impl(c, width, cov_offset, cov_packed, nullptr, exc_cap, exc_index, exc_value, n_exc, rep_offset, rep_s, rep_e, frag_offset,
                             frag_read, frag_begin, frag_end);
}

int raft_hip_fetch_delta4(raft_hip_ctx *c, int64_t *cov_offset, uint8_t *cov_nib, int32_t *cov_anchor, int64_t exc_cap, int64_t *exc_index,
                          int32_t *exc_value, int64_t *n_exc, int64_t *rep_offset, int32_t *rep_s, int32_t *rep_e,
                          int64_t *frag_offset, int32_t *frag_read, int32_t *frag_begin, int32_t *frag_end)
{
    if ((cov_nib != nullptr) != (cov_anchor != nullptr)) return RAFT_HIP_ERR_PARAM;
    return fetch_packed_impl(c, kCovDelta4, cov_offset, cov_nib, cov_anchor, exc_cap, exc_index, exc_value, n_exc, rep_offset, rep_s, rep_e, frag_offset,
                             frag_read, frag_begin, frag_end);
}

int raft_hip_fetch_packed(raft_hip_ctx *c, int64_t *cov_offset, uint8_t *cov8, int64_t exc_cap, int64_t *exc_index,
                          int32_t *exc_value, int64_t *n_exc, int64_t *rep_offset, int32_t *rep_s, int32_t *rep_e,
                          int64_t *frag_offset, int32_t *frag_read, int32_t *frag_begin, int32_t *frag_end)
{
    return raft_hip_fetch_packed_w(c, 1, cov_offset, cov8, exc_cap, exc_index, exc_value, n_exc, rep_offset, rep_s, rep_e, frag_offset,
                                   frag_read, frag_begin, frag_end);
}

// hist[v] = windows of the finished pass with coverage v (cov_hist.hpp), from the form the pass holds: int32, or the codes a width-1 /
// width-2 pass wrote plus its exception list; a delta4 pass is decoded first.  Nothing of the pass is written, no geometry goes out.
int raft_hip_cov_histogram(raft_hip_ctx *c, int64_t *hist, double *kernel_seconds)
{
    static_assert(kCovHistBins == RAFT_HIP_COV_HIST_BINS, "cov_hist.hpp and raft_hip.h disagree");
    if (!c || !hist) return refuse(c, RAFT_HIP_ERR_PARAM, "raft_hip_cov_histogram", kBadArgs);
    if (!c->finished || c->pending_err) return refuse(c, RAFT_HIP_ERR_STATE, "raft_hip_cov_histogram", kNoPass);
    HIP_TRY(c, hipSetDevice(c->device));
    const long long B = c->sum.n_bins;
    // codes as the pass wrote them (a caller that had them re-encoded in another width since holds the int32 array as well: that one then)
    const bool codes = pass_holds_codes(c);
    if (!codes) PHASE(materialise_cov(c));
    else if (c->n_exc > c->exc_cap) { c->last_error = "raft_hip_cov_histogram: the pass's exception list is incomplete"; return RAFT_HIP_ERR_DEVICE; }
    HIP_TRY(c, c->cov_hist.ensure((size_t)kCovHistBins * 8));
    QueryTimer timer(c, kernel_seconds);
    unsigned long long *d_hist = c->cov_hist.as<unsigned long long>();
    HIP_TRY(c, hipMemsetAsync(d_hist, 0, (size_t)kCovHistBins * 8, c->stream));
    PHASE(timer.start());
    if (B > 0) {
        if (!codes) {
            hipLaunchKernelGGL(cov_hist_kernel<int32_t>, dim3(cov_hist_grid(B / kCovHistLaneWindows<int32_t>, B)), dim3(kCovHistThreads), 0, c->stream,
                               c->cov.as<int32_t>(), B, d_hist);
        } else {
            if (c->pass_width == 1)
                hipLaunchKernelGGL(cov_hist_kernel<uint8_t>, dim3(cov_hist_grid(B / kCovHistLaneWindows<uint8_t>, B)), dim3(kCovHistThreads), 0, c->stream,
                                   c->cov8.as<uint8_t>(), B, d_hist);
            else
                hipLaunchKernelGGL(cov_hist_kernel<uint16_t>, dim3(cov_hist_grid(B / kCovHistLaneWindows<uint16_t>, B)), dim3(kCovHistThreads), 0, c->stream,
                                   c->cov8.as<uint16_t>(), B, d_hist);
            if (c->n_exc > 0)       // (complete: raft_hip_finish runs a pass whose list overflowed again)
                hipLaunchKernelGGL(cov_hist_exc_kernel, dim3((unsigned)std::min<long long>((c->n_exc + kCovHistThreads - 1) / kCovHistThreads, kCovHistMaxBlocks)),
                                   dim3(kCovHistThreads), 0, c->stream, c->exc_val.as<int32_t>(), c->n_exc, d_hist);
        }
        HIP_TRY(c, hipGetLastError());
    }
    PHASE(timer.stop());
    HIP_TRY(c, hipMemcpyAsync(hist, d_hist, (size_t)kCovHistBins * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));           // (the one wait of the call: it returns host values)
    PHASE(timer.seconds(kernel_seconds));
    return RAFT_HIP_OK;
}

// Per read: sum and maximum of cov[] over the read's windows and the windows at or above `threshold` (read_stats.hpp), from the form
// the pass holds, as the histogram above.  Nothing of the pass is written, no geometry goes out.
int raft_hip_read_stats(raft_hip_ctx *c, int32_t threshold, int64_t *cov_sum, int32_t *cov_max, int32_t *high_windows, double *kernel_seconds)
{
    if (!c || threshold < 1) return refuse(c, RAFT_HIP_ERR_PARAM, "raft_hip_read_stats", "threshold < 1");
    if (!c->finished || c->pending_err) return refuse(c, RAFT_HIP_ERR_STATE, "raft_hip_read_stats", kNoPass);
    HIP_TRY(c, hipSetDevice(c->device));
    const long long B = c->sum.n_bins;
    const int32_t n_reads = c->sum.n_reads;
    const bool codes = pass_holds_codes(c);
    if (!codes) PHASE(materialise_cov(c));
    else if (c->n_exc > c->exc_cap) { c->last_error = "raft_hip_read_stats: the pass's exception list is incomplete"; return RAFT_HIP_ERR_DEVICE; }
    const size_t n = (size_t)std::max(n_reads, 1);
    HIP_TRY(c, c->rs_sum.ensure(n * 8));
    HIP_TRY(c, c->rs_max.ensure(n * 4));
    HIP_TRY(c, c->rs_high.ensure(n * 4));
    QueryTimer timer(c, kernel_seconds);
    ReadStatsOut out{c->rs_sum.as<unsigned long long>(), c->rs_max.as<int32_t>(), c->rs_high.as<int32_t>()};
    HIP_TRY(c, hipMemsetAsync(out.sum, 0, n * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(out.max, 0, n * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(out.high, 0, n * 4, c->stream));
    PHASE(timer.start());
    if (B > 0 && n_reads > 0) {
        const long long *off = c->cov_off.as<long long>();
        const unsigned thr = (unsigned)threshold;
        if (!codes) {
            hipLaunchKernelGGL(read_stats_kernel<int32_t>, dim3(read_stats_grid(B, kReadStatsLaneWindows<int32_t>)), dim3(kReadStatsThreads), 0, c->stream,
                               c->cov.as<int32_t>(), B, off, n_reads, thr, out);
        } else {
            const unsigned limit = c->pass_width == 1 ? ReadStatsIn<uint8_t>::limit : ReadStatsIn<uint16_t>::limit;
            if (c->pass_width == 1)
                hipLaunchKernelGGL(read_stats_kernel<uint8_t>, dim3(read_stats_grid(B, kReadStatsLaneWindows<uint8_t>)), dim3(kReadStatsThreads), 0, c->stream,
                                   c->cov8.as<uint8_t>(), B, off, n_reads, thr, out);
            else
                hipLaunchKernelGGL(read_stats_kernel<uint16_t>, dim3(read_stats_grid(B, kReadStatsLaneWindows<uint16_t>)), dim3(kReadStatsThreads), 0, c->stream,
                                   c->cov8.as<uint16_t>(), B, off, n_reads, thr, out);
            if (c->n_exc > 0)       // (complete: raft_hip_finish runs a pass whose list overflowed again)
                hipLaunchKernelGGL(read_stats_exc_kernel, dim3((unsigned)std::min<long long>((c->n_exc + 255) / 256, 4096)), dim3(256), 0, c->stream,
                                   c->exc_idx.as<long long>(), c->exc_val.as<int32_t>(), c->n_exc, off, n_reads, limit, thr, out);
        }
        HIP_TRY(c, hipGetLastError());
    }
    PHASE(timer.stop());
    PHASE(queue_copies(c, {{cov_sum, out.sum, (size_t)n_reads * 8}, {cov_max, out.max, (size_t)n_reads * 4}, {high_windows, out.high, (size_t)n_reads * 4}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));           // (the one wait of the call)
    PHASE(timer.seconds(kernel_seconds));
    return RAFT_HIP_OK;
}

// What the record stream says about each read (census.hpp): intervals per read under the final flag `symmetric`, contained flags.
// Independent of any pass: the call reads its arguments and writes buffers of its own.
static int census_run(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_len, const RecordCols &rec, int32_t symmetric,
                      int32_t *intervals, uint8_t *contained, int64_t *n_contained, int64_t *error_index, double *kernel_seconds)
{
    const size_t n = (size_t)std::max(n_reads, 1);
    HIP_TRY(c, c->cen_cnt.ensure(n * 4));
    HIP_TRY(c, c->cen_flags.ensure(n * 4));
    HIP_TRY(c, c->cen_out.ensure(n));
    HIP_TRY(c, c->cen_ctl.ensure(16));
    QueryTimer timer(c, kernel_seconds);
    unsigned long long *ctl = c->cen_ctl.as<unsigned long long>();        // [0] first bad record, [1] reads with a flag
    HIP_TRY(c, hipMemsetAsync(c->cen_cnt.p, 0, n * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->cen_flags.p, 0, n * 4, c->stream));
    PHASE(clear_ctl(c, ctl, 2));
    PHASE(timer.start());
    const int64_t n_rec = rec.n_rec;
    if (n_rec > 0) {
        CensusArgs A{d_len, rec.col[0], rec.col[1], rec.col[2], rec.col[3], rec.col[4], rec.col[5], (long long)n_rec, n_reads,
                     symmetric ? 1 : 0, c->cen_cnt.as<unsigned>(), c->cen_flags.as<unsigned>(), ctl};
        if (aligned16(rec)) hipLaunchKernelGGL(census_kernel<true>, dim3(stream_grid(n_rec)), dim3(kStreamThreads), 0, c->stream, A);
        else hipLaunchKernelGGL(census_kernel<false>, dim3(stream_grid(n_rec)), dim3(kStreamThreads), 0, c->stream, A);
    }
    if (n_reads > 0)
        hipLaunchKernelGGL(census_pack_kernel, dim3((unsigned)std::min<long long>(((long long)n_reads + 255) / 256, 1024)), dim3(256), 0, c->stream,
                           c->cen_flags.as<unsigned>(), n_reads, c->cen_out.as<uint8_t>(), ctl + 1);
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[2] = {0, 0};
    PHASE(read_ctl(c, ctl, h_ctl, 2));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(kernel_seconds));
    PHASE(first_bad_record(c, h_ctl[0], error_index, "census: a record names a read id outside [0, n_reads)"));
    if (n_contained) *n_contained = (int64_t)h_ctl[1];
    PHASE(queue_copies(c, {{intervals, c->cen_cnt.p, (size_t)n_reads * 4}, {contained, c->cen_out.p, (size_t)n_reads}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RAFT_HIP_OK;
}

// the record columns as the census reads them: under `symmetric` ts / te are not looked at, whatever the caller passed
static RecordCols census_cols(int64_t n_rec, const int32_t *qid, const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts,
                              const int32_t *te, int32_t symmetric)
{
    return RecordCols{n_rec, {qid, qs, qe, tid, symmetric ? nullptr : ts, symmetric ? nullptr : te}};
}

static bool census_args_ok(const raft_hip_ctx *c, int32_t n_reads, const int32_t *len, const RecordCols &rec, int32_t symmetric)
{
    if (!c || n_reads < 0 || rec.n_rec < 0 || (n_reads > 0 && !len)) return false;
    return record_cols_ok(rec, symmetric != 0, TargetCols::unread_if_symmetric);
}

int raft_hip_census_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid, const int32_t *d_qs,
                           const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te, int32_t symmetric,
                           int32_t *intervals, uint8_t *contained, int64_t *n_contained, int64_t *error_index, double *kernel_seconds)
{
    const RecordCols rec = census_cols(n_rec, d_qid, d_qs, d_qe, d_tid, d_ts, d_te, symmetric);
    if (!census_args_ok(c, n_reads, d_read_len, rec, symmetric)) return refuse(c, RAFT_HIP_ERR_PARAM, "census", kBadArgs);
    HIP_TRY(c, hipSetDevice(c->device));
    return census_run(c, n_reads, d_read_len, rec, symmetric, intervals, contained, n_contained, error_index, kernel_seconds);
}

// The same from host arrays, staged through the census's own buffers (cen_len, cen_col).
int raft_hip_census_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid, const int32_t *qs,
                         const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te, int32_t symmetric,
                         int32_t *intervals, uint8_t *contained, int64_t *n_contained, int64_t *error_index, double *kernel_seconds)
{
    RecordCols rec = census_cols(n_rec, qid, qs, qe, tid, ts, te, symmetric);
    if (!census_args_ok(c, n_reads, read_len, rec, symmetric)) return refuse(c, RAFT_HIP_ERR_PARAM, "census", kBadArgs);
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(stage_host(c, c->cen_len, read_len, (size_t)n_reads, &read_len));
    PHASE(stage_columns(c, c->cen_col, rec));
    return census_run(c, n_reads, read_len, rec, symmetric, intervals, contained, n_contained, error_index, kernel_seconds);
}

// The estimate read from a histogram: the mode of the covered, unclamped bins smoothed over three neighbours (see raft_hip.h).
// Pure host arithmetic; sums are kept in 128 bits so that no count a caller can pass wraps.
int raft_hip_estimate_coverage(const int64_t *hist, int32_t n_hist, raft_hip_cov_estimate *out)
{
    if (!hist || !out || n_hist < 3) return RAFT_HIP_ERR_PARAM;
    typedef unsigned __int128 u128;
    u128 total = 0, weighted = 0;
    for (int32_t v = 0; v < n_hist; ++v) {
        if (hist[v] < 0) return RAFT_HIP_ERR_PARAM;
        total += (u128)hist[v];
        weighted += (u128)hist[v] * (u128)v;
    }
    if (total > (u128)INT64_MAX) return RAFT_HIP_ERR_TOO_LARGE;
    const int n = n_hist;
    auto c = [&](int v) -> u128 { return v >= 1 && v <= n - 2 ? (u128)hist[v] : (u128)0; };
    u128 best = 0;
    int32_t est = 0;
    for (int v = 1; v <= n - 2; ++v) {
        const u128 s = c(v - 1) + c(v) + c(v + 1);
        if (s > best) { best = s; est = v; }          // (strictly greater: the smallest v of a tie stays)
    }
    const u128 covered = total - (u128)hist[0];
    int32_t median = 0;
    if (covered > 0) {
        u128 run = 0;
        for (int v = 1; v < n; ++v) {
            run += (u128)hist[v];
            if (2 * run >= covered) { median = v; break; }
        }
    }
    out->est_cov = est;
    out->median = median;
    out->windows = (int64_t)total;
    out->windows_covered = (int64_t)covered;
    out->windows_clamped = hist[n - 1];
    out->mean = total > 0 ? (double)weighted / (double)total : 0.0;
    return RAFT_HIP_OK;
}

int raft_hip_last_timing(raft_hip_ctx *c, double *pileup_seconds, double *pass_seconds)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (!c->finished) return RAFT_HIP_ERR_STATE;
    HIP_TRY(c, hipEventSynchronize(c->ev_pass1));          // (finish may have seen the pass's number before the runtime saw its last event)
    float ms = 0.f;
    if (pileup_seconds) { HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_pile0, c->ev_pile1)); *pileup_seconds = ms * 1e-3; }
    if (pass_seconds) { HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_pass0, c->ev_pass1)); *pass_seconds = ms * 1e-3; }
    return RAFT_HIP_OK;
}

int raft_hip_selftest(int device_id)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return RAFT_HIP_ERR_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return RAFT_HIP_ERR_DEVICE;
    const int n = 256;
    int h_in[n], h_a[n], h_b[n];
    unsigned long long h_bal[n / 64];
    unsigned s = 12345u;
    for (int i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h_in[i] = (int)(s >> 20) - 2048; }
    int *d_in = nullptr, *d_a = nullptr, *d_b = nullptr;
    unsigned long long *d_bal = nullptr;
    int rc = RAFT_HIP_ERR_DEVICE;
    if (hipMalloc(&d_in, sizeof h_in) == hipSuccess && hipMalloc(&d_a, sizeof h_a) == hipSuccess &&
        hipMalloc(&d_b, sizeof h_b) == hipSuccess && hipMalloc(&d_bal, sizeof h_bal) == hipSuccess &&
        hipMemcpy(d_in, h_in, sizeof h_in, hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(n), 0, 0, d_in, d_a, d_b, d_bal);
        if (hipMemcpy(h_a, d_a, sizeof h_a, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(h_b, d_b, sizeof h_b, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(h_bal, d_bal, sizeof h_bal, hipMemcpyDeviceToHost) == hipSuccess) {
            rc = RAFT_HIP_OK;
            for (int w = 0; w < n / 64; ++w) {
                int run = 0;
                unsigned long long bal = 0;
                for (int l = 0; l < 64; ++l) {
                    run += h_in[w * 64 + l];
                    if (h_in[w * 64 + l] & 1) bal |= 1ull << l;
                    if (h_a[w * 64 + l] != run || h_b[w * 64 + l] != run) rc = 100 + w;
                }
                if (bal != h_bal[w]) rc = 200 + w;
            }
        }
    }
    (void)hipFree(d_in); (void)hipFree(d_a); (void)hipFree(d_b); (void)hipFree(d_bal);
    return rc;
}

} // extern "C"
