// low_cov_lib.hip -- libraft_hip_low.so: raft_hip_low_coverage (include/raft_hip_low.h), the low-coverage runs of a finished pass.
//
// A library of its own beside libraft_hip.so: the set of entry points of include/raft_hip.h is closed (ABI 11), and this query needs
// nothing of the engine but the context it is handed -- the buffers a finished pass left (engine_ctx.hpp), the stream, and buffers
// registered with the context like every other (lc_*, and the queries' shared decoded coverage q_cov).  Both libraries are built from
// this tree against the same engine_ctx.hpp, and raft_hip_low_abi() says which ABI version of the engine this one was built beside.
#include "cov_decode.hpp"
#include "../../include/raft_hip_low.h"
#include "low_cov.hpp"

#include <algorithm>

extern "C" {

int raft_hip_low_abi(void) { return RAFT_HIP_ABI_VERSION; }

// The low-coverage runs of every read (low_cov.hpp): windows with cov[w] <= low_cov, as CSR by read, with per-read counts, class
// flags and totals.  Reads the form the pass holds, as the two calls above; nothing of the pass is written, no geometry goes out.
// Two waits: one for the run total, which sizes the run arrays, and the one at the end.
int raft_hip_low_coverage(raft_hip_ctx *c, int32_t low_cov, int32_t uncovered_permille, int64_t run_cap, int64_t *low_offset, int32_t *low_s,
                          int32_t *low_e, int32_t *low_windows, uint8_t *low_flags, raft_hip_low_summary *sum, double *kernel_seconds)
{
    if (!c || low_cov < 0 || uncovered_permille < 0 || uncovered_permille > 1000) return refuse(c, RAFT_HIP_ERR_PARAM, "raft_hip_low_coverage", kBadArgs);
    if (!c->finished || c->pending_err) return refuse(c, RAFT_HIP_ERR_STATE, "raft_hip_low_coverage", kNoPass);
    HIP_TRY(c, hipSetDevice(c->device));
    const long long B = c->sum.n_bins;
    const int32_t n_reads = c->sum.n_reads;
    const bool pass_codes = pass_holds_codes(c);
    if (pass_codes && c->n_exc > c->exc_cap) { c->last_error = "raft_hip_low_coverage: the pass's exception list is incomplete"; return RAFT_HIP_ERR_DEVICE; }
    // codes in place while low_cov lies below the code's limit: a code at the limit is then not low, whatever its window holds
    const bool codes = pass_codes && (long long)low_cov < (c->pass_width == 1 ? 255ll : 65535ll);
    const int32_t *cov32 = nullptr;
    if (!codes) PHASE(query_cov(c, "raft_hip_low_coverage", &cov32));
    const long long n_words = (B + kLowWordWindows - 1) / kLowWordWindows;
    const long long n_tiles = (n_words + kLowTileWords - 1) / kLowTileWords;
    const size_t n = (size_t)std::max(n_reads, 1);
    HIP_TRY(c, c->lc_bad.ensure((size_t)std::max(n_words, 1LL) * 8));
    HIP_TRY(c, c->lc_rs.ensure((size_t)std::max(n_words, 1LL) * 8));
    HIP_TRY(c, c->lc_tile_cnt.ensure((size_t)std::max(n_tiles, 1LL) * 4));
    HIP_TRY(c, c->lc_tile_base.ensure((size_t)std::max(n_tiles, 1LL) * 8));
    HIP_TRY(c, c->lc_ctl.ensure((size_t)kLowCtlWords * 8));
    HIP_TRY(c, c->lc_win.ensure(n * 4)); HIP_TRY(c, c->lc_bases.ensure(n * 4)); HIP_TRY(c, c->lc_flagw.ensure(n * 4));
    HIP_TRY(c, c->lc_flags.ensure(n)); HIP_TRY(c, c->lc_off.ensure((n + 1) * 8));
    HIP_TRY(c, c->len_seen.ensure(n * 4));                 // (a context whose passes never saw a read has none)
    QueryTimer timer(c, kernel_seconds);
    unsigned long long *bad = c->lc_bad.as<unsigned long long>(), *rs = c->lc_rs.as<unsigned long long>(), *ctl = c->lc_ctl.as<unsigned long long>();
    const long long *off = c->cov_off.as<long long>();
    LowReads acc{c->lc_win.as<unsigned>(), c->lc_bases.as<unsigned>(), c->lc_flagw.as<unsigned>()};
    HIP_TRY(c, hipMemsetAsync(rs, 0, (size_t)std::max(n_words, 1LL) * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(ctl, 0, (size_t)kLowCtlWords * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(acc.windows, 0, n * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(acc.bases, 0, n * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(acc.flag_words, 0, n * 4, c->stream));
    double head_seconds = 0.0, tail_seconds = 0.0;      // (two spans: the host sizes the run arrays in between)
    PHASE(timer.start());
    if (B > 0 && n_reads > 0) {
        const unsigned thr = (unsigned)low_cov;
        auto mark_grid = [&](int lane_windows) { return dim3((unsigned)((n_words * kLowWordWindows / lane_windows + kLowMarkGroups - 1) / kLowMarkGroups)); };
        if (!codes)
            hipLaunchKernelGGL(low_mark_kernel<int32_t>, mark_grid(kLowLaneWindows<int32_t>), dim3(kLowThreads), 0, c->stream, cov32, B, thr,
                               (void *)bad, n_words * kLowWordWindows / kLowLaneWindows<int32_t>);
        else if (c->pass_width == 1)
            hipLaunchKernelGGL(low_mark_kernel<uint8_t>, mark_grid(kLowLaneWindows<uint8_t>), dim3(kLowThreads), 0, c->stream, c->cov8.as<uint8_t>(), B, thr,
                               (void *)bad, n_words * kLowWordWindows / kLowLaneWindows<uint8_t>);
        else
            hipLaunchKernelGGL(low_mark_kernel<uint16_t>, mark_grid(kLowLaneWindows<uint16_t>), dim3(kLowThreads), 0, c->stream, c->cov8.as<uint16_t>(), B, thr,
                               (void *)bad, n_words * kLowWordWindows / kLowLaneWindows<uint16_t>);
        hipLaunchKernelGGL(low_read_starts_kernel, dim3((unsigned)(((long long)n_reads + kLowThreads - 1) / kLowThreads)), dim3(kLowThreads), 0, c->stream,
                           off, n_reads, rs);
        hipLaunchKernelGGL(low_count_kernel, dim3((unsigned)n_tiles), dim3(kLowThreads), 0, c->stream, bad, rs, n_words, c->lc_tile_cnt.as<int32_t>());
        hipLaunchKernelGGL(low_prefix_kernel, dim3(1), dim3(kLowPrefixThreads), 0, c->stream, c->lc_tile_cnt.as<int32_t>(), n_tiles,
                           c->lc_tile_base.as<long long>(), ctl);
        HIP_TRY(c, hipGetLastError());
    }
    PHASE(timer.stop());
    unsigned long long h_ctl[kLowCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, 1));
    HIP_TRY(c, hipStreamSynchronize(c->stream));           // (the run total: it sizes the run arrays)
    PHASE(timer.seconds(&head_seconds));
    const long long n_runs = (long long)h_ctl[0];
    if (n_runs < 0 || n_runs > (B + n_reads) / 2) { c->last_error = "raft_hip_low_coverage: more runs than windows and reads allow"; return RAFT_HIP_ERR_DEVICE; }
    const size_t nr = (size_t)std::max(n_runs, 1LL);
    HIP_TRY(c, c->lc_s.ensure(nr * 4)); HIP_TRY(c, c->lc_e.ensure(nr * 4)); HIP_TRY(c, c->lc_read.ensure(nr * 4));
    LowRuns runs{c->lc_s.as<int32_t>(), c->lc_e.as<int32_t>(), c->lc_read.as<int32_t>()};
    PHASE(timer.start());
    if (n_runs > 0) {
        hipLaunchKernelGGL(low_fill_kernel, dim3((unsigned)n_tiles), dim3(kLowThreads), 0, c->stream, bad, rs, n_words, c->lc_tile_base.as<long long>(), off,
                           c->len_seen.as<int32_t>(), n_reads, c->prm.reso, n_runs, runs, ctl);
        hipLaunchKernelGGL(low_runs_kernel, dim3((unsigned)((n_runs + kLowThreads - 1) / kLowThreads)), dim3(kLowThreads), 0, c->stream, runs, n_runs, off,
                           n_reads, c->prm.reso, acc, ctl);
    }
    hipLaunchKernelGGL(low_reads_kernel, dim3((unsigned)(((long long)n_reads + 1 + kLowThreads - 1) / kLowThreads)), dim3(kLowThreads), 0, c->stream,
                       runs.read, n_runs, c->len_seen.as<int32_t>(), n_reads, uncovered_permille, acc, c->lc_off.as<long long>(),
                       c->lc_flags.as<uint8_t>(), ctl);
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    PHASE(read_ctl(c, ctl, h_ctl, kLowCtlWords));
    const bool fits = n_runs <= run_cap;
    PHASE(queue_copies(c, {{low_offset, c->lc_off.p, ((size_t)n_reads + 1) * 8}, {low_windows, acc.windows, (size_t)n_reads * 4},
                           {low_flags, c->lc_flags.p, (size_t)n_reads}}));
    if (fits) PHASE(queue_copies(c, {{low_s, runs.s, (size_t)n_runs * 4}, {low_e, runs.e, (size_t)n_runs * 4}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(&tail_seconds));
    if (kernel_seconds) *kernel_seconds = head_seconds + tail_seconds;
    if (h_ctl[6]) { c->last_error = "raft_hip_low_coverage: a run's rank fell outside the run total"; return RAFT_HIP_ERR_DEVICE; }
    if (sum) {
        sum->n_runs = n_runs; sum->low_windows = (int64_t)h_ctl[1]; sum->low_bases = (int64_t)h_ctl[2];
        sum->reads_with_runs = (int64_t)h_ctl[3]; sum->reads_interior = (int64_t)h_ctl[4]; sum->reads_uncovered = (int64_t)h_ctl[5];
    }
    if (!fits && (low_s || low_e)) return RAFT_HIP_ERR_TOO_LARGE;
    return RAFT_HIP_OK;
}

} // extern "C"
