// repeat_stats_lib.hip -- libraft_hip_rst.so: raft_hip_repeat_stats_device / _host (include/raft_hip_rst.h), one row per repeat run.
//
// A library of its own beside libraft_hip.so, as libraft_hip_low.so, libraft_hip_ovl.so and libraft_hip_frag.so are: the set of entry
// points of include/raft_hip.h is closed (ABI 11), and this query needs nothing of the engine but the context it is handed -- the
// coverage and the repeat arrays a finished pass left (engine_ctx.hpp), the stream, and buffers of its own registered with the
// context like every other (rst_*).
#include "engine_ctx.hpp"
#include "../../include/raft_hip_rst.h"
#include "pack.hpp"
#include "repeat_stats.hpp"

#include <algorithm>

static_assert(kRstEmpty == RAFT_HIP_RST_EMPTY && kRstAtStart == RAFT_HIP_RST_AT_START && kRstAtEnd == RAFT_HIP_RST_AT_END, "the kernels write the header's bits");

namespace {

#define PHASE(expr)                                              \
    do {                                                         \
        const int rc_ = (expr);                                  \
        if (rc_ != RAFT_HIP_OK) return rc_;                      \
    } while (0)

inline unsigned grid_for(long long n, long long per_block, long long cap)
{
    return (unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, cap));
}

// a destination the caller left NULL, or nothing to copy, is skipped
int queue_copy(raft_hip_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (dst && bytes) HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return RAFT_HIP_OK;
}

struct RstCall {
    int32_t n_reads; const int32_t *len; int64_t n_rec; const int32_t *col[6];
    int32_t symmetric;
    int64_t n_rep; const int64_t *rep_off; const int32_t *rep_s, *rep_e;      // device arrays, or all NULL with n_rep = -1: the context's pass
    int32_t threshold;
    int32_t *cnt[3];                                                          // touch, span, inside
    int32_t *win[4];                                                          // windows, min, max, high
    int64_t *cov_sum; uint8_t *flags;
    raft_hip_rst_summary *sum; int64_t *error_index; double *kernel_seconds;
};

// what both forms check before anything is staged: counts, columns, the three repeat arrays, the state the call needs
int check_call(raft_hip_ctx *c, const RstCall &a)
{
    if (!c || a.n_reads < 0 || a.n_rec < 0 || a.threshold < 0 || (a.n_reads > 0 && !a.len)) return RAFT_HIP_ERR_PARAM;
    if (a.n_rec > 0 && (!a.col[0] || !a.col[1] || !a.col[2] || !a.col[3])) return RAFT_HIP_ERR_PARAM;
    if ((a.col[4] == nullptr) != (a.col[5] == nullptr)) return RAFT_HIP_ERR_PARAM;
    if (a.n_rec > 0 && !a.symmetric && !a.col[4]) return RAFT_HIP_ERR_PARAM;
    if (a.threshold == 0 && (a.win[0] || a.win[1] || a.win[2] || a.win[3] || a.cov_sum)) return RAFT_HIP_ERR_PARAM;
    const int given = (a.rep_off ? 1 : 0) + (a.rep_s ? 1 : 0) + (a.rep_e ? 1 : 0);
    const bool own = given == 0 && a.n_rep == -1;
    if (!own) {
        if (a.n_rep < 0 || !a.rep_off) return RAFT_HIP_ERR_PARAM;
        if (a.n_rep > 0 ? given != 3 : (given != 1 && given != 3)) return RAFT_HIP_ERR_PARAM;    // (no run: rep_s / rep_e have nothing to point at)
    }
    if (a.n_rec >= (int64_t(1) << 30) || a.n_rep >= (int64_t(1) << 31) - 1) return RAFT_HIP_ERR_TOO_LARGE;
    if (own || a.threshold >= 1) {                            // the context's own finished pass: its annotation, its coverage
        if (!c->finished || c->pending_err) return RAFT_HIP_ERR_STATE;
        if (a.n_reads != c->sum.n_reads) return RAFT_HIP_ERR_PARAM;
        if (own && c->sum.n_repeats >= (int64_t(1) << 31) - 1) return RAFT_HIP_ERR_TOO_LARGE;
    }
    return RAFT_HIP_OK;
}

// The int32 array of the last pass, as low_cov_lib.hip finds it: the context's own when it holds one (a pass that wrote int32, or one
// somebody fetched), else decoded from the codes or four-bit steps into a buffer of this query's (rst_cov) with the kernels of
// pack.hpp in the order engine.hip's materialise_cov runs them.  Nothing of the engine's is allocated, written or marked here.
int int32_cov(raft_hip_ctx *c, const int32_t **out)
{
    if (c->cov_valid) { *out = c->cov.as<int32_t>(); return RAFT_HIP_OK; }
    const bool pass_codes = (c->pass_width == 1 || c->pass_width == 2) && c->packed_width == c->pass_width;
    if (pass_codes && c->n_exc > c->exc_cap) { c->last_error = "repeat_stats: the pass's exception list is incomplete"; return RAFT_HIP_ERR_DEVICE; }
    const long long B = c->sum.n_bins;
    HIP_TRY(c, c->rst_cov.ensure((size_t)std::max(B, 1LL) * 4));
    int32_t *cov = c->rst_cov.as<int32_t>();
    *out = cov;
    if (B > 0) {
        const bool d4 = c->pass_width == kCovDelta4;
        if (d4) {
            if (c->d4_shift != 0) return RAFT_HIP_ERR_STATE;      // (a pipeline lane's chunk: its blocks do not begin at its first window)
            HIP_TRY(c, c->rst_abs.ensure(((size_t)B / 32 + 2) * 4));
            hipLaunchKernelGGL(delta4_expand_kernel, dim3(grid_for(B / 32, 256, 256 * 16)), dim3(256), 0, c->stream,
                               c->cov8.as<uint8_t>(), B, cov, c->rst_abs.as<unsigned>());
        } else if (c->pass_width == 1)
            hipLaunchKernelGGL(unpack_cov_kernel<uint8_t>, dim3(grid_for(B / 4, 256, 256 * 16)), dim3(256), 0, c->stream, c->cov8.as<uint8_t>(), B, cov);
        else if (c->pass_width == 2)
            hipLaunchKernelGGL(unpack_cov_kernel<uint16_t>, dim3(grid_for(B / 4, 256, 256 * 16)), dim3(256), 0, c->stream, c->cov8.as<uint16_t>(), B, cov);
        else { c->last_error = "repeat_stats: the pass holds neither int32 nor an encoding"; return RAFT_HIP_ERR_STATE; }
        if (c->n_exc > 0)      // the listed windows, over what the codes gave (delta4: before the walk that adds the steps up)
            hipLaunchKernelGGL(scatter_exceptions_kernel, dim3((unsigned)std::min<long long>((c->n_exc + 255) / 256, 4096)), dim3(256), 0, c->stream,
                               c->exc_idx.as<long long>(), c->exc_val.as<int32_t>(), c->n_exc, cov);
        if (d4)
            hipLaunchKernelGGL(delta4_walk_kernel, dim3(grid_for(B / kD4Block, 256, 256 * 16)), dim3(256), 0, c->stream,
                               B, c->cov_anchor.as<int32_t>(), c->rst_abs.as<unsigned>(), cov);
        HIP_TRY(c, hipGetLastError());
    }
    return RAFT_HIP_OK;
}

int rst_run(raft_hip_ctx *c, const RstCall &a)
{
    const bool own = a.n_rep == -1, with_cov = a.threshold >= 1;
    const long long *rep_off = own ? c->rep_off.as<long long>() : reinterpret_cast<const long long *>(a.rep_off);
    const int32_t *rep_s = own ? c->rep_s.as<int32_t>() : a.rep_s, *rep_e = own ? c->rep_e.as<int32_t>() : a.rep_e;
    const long long n_rep = own ? c->sum.n_repeats : a.n_rep;
    const size_t n = (size_t)std::max(a.n_reads, 1), nr = (size_t)std::max<long long>(n_rep, 1);
    HIP_TRY(c, c->rst_digest.ensure(n * sizeof(RstDigest)));
    HIP_TRY(c, c->rst_run_read.ensure(nr * 4));
    HIP_TRY(c, c->rst_slot.ensure(nr * sizeof(RstSlot)));
    for (DevBuf &b : c->rst_cnt) HIP_TRY(c, b.ensure(nr * 4));
    HIP_TRY(c, c->rst_flags.ensure(nr));
    HIP_TRY(c, c->rst_ctl.ensure((size_t)kRstCtlWords * 8));
    if (with_cov) {
        for (DevBuf &b : c->rst_win) HIP_TRY(c, b.ensure(nr * 4));
        HIP_TRY(c, c->rst_sum.ensure(nr * 8));
    }
    if (a.kernel_seconds && !c->ev_hist0) { HIP_TRY(c, hipEventCreate(&c->ev_hist0)); HIP_TRY(c, hipEventCreate(&c->ev_hist1)); }
    unsigned long long *ctl = c->rst_ctl.as<unsigned long long>();
    int32_t *run_read = c->rst_run_read.as<int32_t>();
    RstSlot *slot = c->rst_slot.as<RstSlot>();
    if (a.kernel_seconds) HIP_TRY(c, hipEventRecord(c->ev_hist0, c->stream));
    HIP_TRY(c, hipMemsetAsync(slot, 0, nr * sizeof(RstSlot), c->stream));
    HIP_TRY(c, hipMemsetAsync(ctl, 0xFF, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(ctl + 1, 0, (size_t)(kRstCtlWords - 1) * 8, c->stream));
    const int32_t *cov = nullptr;
    if (with_cov) PHASE(int32_cov(c, &cov));
    if (a.n_reads > 0 || !own)
        hipLaunchKernelGGL(rst_digest_kernel, dim3((unsigned)(((long long)a.n_reads + 1 + 255) / 256)), dim3(256), 0, c->stream, rep_off, rep_s, rep_e,
                           a.n_reads, n_rep, c->rst_digest.as<RstDigest>(), run_read, ctl);
    if (a.n_rec > 0) {                                        // (without a run too: the ids are checked)
        RstArgs A{a.col[0], a.col[1], a.col[2], a.col[3], a.col[4], a.col[5], (long long)a.n_rec, a.n_reads, a.symmetric ? 1 : 0,
                  rep_s, rep_e, c->rst_digest.as<RstDigest>(), slot, ctl};
        uintptr_t bits = 0;
        for (int k = 0; k < 6; ++k) bits |= reinterpret_cast<uintptr_t>(a.col[k]);
        if (bits & 15) hipLaunchKernelGGL(rst_side_kernel<false>, dim3(rst_grid(a.n_rec)), dim3(kRstThreads), 0, c->stream, A);
        else hipLaunchKernelGGL(rst_side_kernel<true>, dim3(rst_grid(a.n_rec)), dim3(kRstThreads), 0, c->stream, A);
    }
    RstCovOut co{c->rst_win[0].as<int32_t>(), c->rst_win[1].as<int32_t>(), c->rst_win[2].as<int32_t>(), c->rst_win[3].as<int32_t>(), c->rst_sum.as<long long>()};
    if (n_rep > 0) {
        if (with_cov)
            hipLaunchKernelGGL(rst_cov_kernel, dim3(rst_cov_grid(n_rep)), dim3(kRstCovThreads), 0, c->stream, cov, c->cov_off.as<long long>(), rep_s, rep_e,
                               run_read, n_rep, c->prm.reso, a.threshold, ctl, co);
        RstRunsArgs R{slot, rep_s, rep_e, run_read, a.len, n_rep, with_cov ? co.windows : nullptr, co.cov_sum, c->rst_cnt[0].as<int32_t>(),
                      c->rst_cnt[1].as<int32_t>(), c->rst_cnt[2].as<int32_t>(), c->rst_flags.as<uint8_t>(), ctl};
        hipLaunchKernelGGL(rst_runs_kernel, dim3(grid_for(n_rep, 256, 2048)), dim3(256), 0, c->stream, R);
    }
    HIP_TRY(c, hipGetLastError());
    if (a.kernel_seconds) HIP_TRY(c, hipEventRecord(c->ev_hist1, c->stream));
    unsigned long long h_ctl[kRstCtlWords] = {};
    HIP_TRY(c, hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.kernel_seconds) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_hist0, c->ev_hist1));
        *a.kernel_seconds = ms * 1e-3;
    }
    if (h_ctl[kRstBadOffsets]) {
        c->last_error = "repeat_stats: rep_offset does not begin at 0, ascend and end at n_rep";
        return RAFT_HIP_ERR_PARAM;
    }
    if (h_ctl[kRstFirstBad] != ~0ull) {
        if (a.error_index) *a.error_index = (int64_t)h_ctl[kRstFirstBad];
        c->last_error = "repeat_stats: a record names a read id outside [0, n_reads)";
        return RAFT_HIP_ERR_READ_ID;
    }
    if (a.error_index) *a.error_index = -1;
    for (int k = 0; k < 3; ++k) PHASE(queue_copy(c, a.cnt[k], c->rst_cnt[k].p, (size_t)n_rep * 4));
    PHASE(queue_copy(c, a.flags, c->rst_flags.p, (size_t)n_rep));
    if (with_cov) {
        for (int k = 0; k < 4; ++k) PHASE(queue_copy(c, a.win[k], c->rst_win[k].p, (size_t)n_rep * 4));
        PHASE(queue_copy(c, a.cov_sum, c->rst_sum.p, (size_t)n_rep * 8));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum) {
        const unsigned long long *t = h_ctl + kRstTotals;
        a.sum->n_runs = n_rep;
        a.sum->runs_empty = (int64_t)t[0]; a.sum->runs_interior = (int64_t)t[1]; a.sum->runs_touched = (int64_t)t[2];
        a.sum->runs_spanned = (int64_t)t[3]; a.sum->interior_spanned = (int64_t)t[4];
        a.sum->sides_touch = (int64_t)t[5]; a.sum->sides_span = (int64_t)t[6]; a.sum->sides_inside = (int64_t)t[7];
        a.sum->windows = (int64_t)t[8]; a.sum->cov_sum = (int64_t)t[9];
    }
    return RAFT_HIP_OK;
}

RstCall make_call(int32_t n_reads, const int32_t *len, const raft_hip_records *rec, int32_t symmetric, int64_t n_rep, const int64_t *rep_off,
                  const int32_t *rep_s, const int32_t *rep_e, int32_t threshold, int32_t *touch, int32_t *span, int32_t *inside, int32_t *windows,
                  int32_t *cov_min, int32_t *cov_max, int32_t *high, int64_t *cov_sum, uint8_t *flags, raft_hip_rst_summary *sum, int64_t *error_index,
                  double *kernel_seconds)
{
    RstCall a{n_reads, len, 0, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, symmetric, n_rep, rep_off, rep_s, rep_e, threshold,
              {touch, span, inside}, {windows, cov_min, cov_max, high}, cov_sum, flags, sum, error_index, kernel_seconds};
    if (rec && rec->n_rec != 0) {                            // (NULL or no records: every count is 0)
        a.n_rec = rec->n_rec;
        const int32_t *col[6] = {rec->d_qid, rec->d_qs, rec->d_qe, rec->d_tid, rec->d_ts, rec->d_te};
        for (int k = 0; k < 6; ++k) a.col[k] = col[k];
    }
    return a;
}

} // namespace

extern "C" {

int raft_hip_rst_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_repeat_stats_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, const raft_hip_records *records, int32_t symmetric,
                                 int64_t n_rep, const int64_t *d_rep_offset, const int32_t *d_rep_s, const int32_t *d_rep_e, int32_t threshold,
                                 int32_t *run_touch, int32_t *run_span, int32_t *run_inside, int32_t *run_windows, int32_t *run_cov_min,
                                 int32_t *run_cov_max, int32_t *run_high, int64_t *run_cov_sum, uint8_t *run_flags, raft_hip_rst_summary *sum,
                                 int64_t *error_index, double *kernel_seconds)
{
    const RstCall a = make_call(n_reads, d_read_len, records, symmetric, n_rep, d_rep_offset, d_rep_s, d_rep_e, threshold, run_touch, run_span, run_inside,
                                run_windows, run_cov_min, run_cov_max, run_high, run_cov_sum, run_flags, sum, error_index, kernel_seconds);
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return rst_run(c, a);
}

// The same from host arrays, staged through buffers of the context that no pass uses (rst_len, rst_col, rst_rep_*).
int raft_hip_repeat_stats_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, const raft_hip_records *records, int32_t symmetric,
                               int64_t n_rep, const int64_t *rep_offset, const int32_t *rep_s, const int32_t *rep_e, int32_t threshold,
                               int32_t *run_touch, int32_t *run_span, int32_t *run_inside, int32_t *run_windows, int32_t *run_cov_min,
                               int32_t *run_cov_max, int32_t *run_high, int64_t *run_cov_sum, uint8_t *run_flags, raft_hip_rst_summary *sum,
                               int64_t *error_index, double *kernel_seconds)
{
    RstCall a = make_call(n_reads, read_len, records, symmetric, n_rep, rep_offset, rep_s, rep_e, threshold, run_touch, run_span, run_inside,
                          run_windows, run_cov_min, run_cov_max, run_high, run_cov_sum, run_flags, sum, error_index, kernel_seconds);
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    auto stage = [&](DevBuf &buf, const void *src, size_t count, size_t elem, const void **dev) -> int {
        HIP_TRY(c, buf.ensure(std::max<size_t>(count, 1) * elem));
        if (count > 0 && src) HIP_TRY(c, hipMemcpyAsync(buf.p, src, count * elem, hipMemcpyHostToDevice, c->stream));
        *dev = buf.p;
        return RAFT_HIP_OK;
    };
    PHASE(stage(c->rst_len, read_len, (size_t)n_reads, 4, reinterpret_cast<const void **>(&a.len)));
    for (int k = 0; k < 6; ++k)
        if (a.col[k]) PHASE(stage(c->rst_col[k], a.col[k], (size_t)a.n_rec, 4, reinterpret_cast<const void **>(&a.col[k])));
    if (n_rep != -1) {
        PHASE(stage(c->rst_rep_off, rep_offset, (size_t)n_reads + 1, 8, reinterpret_cast<const void **>(&a.rep_off)));
        PHASE(stage(c->rst_rep_s, rep_s, (size_t)n_rep, 4, reinterpret_cast<const void **>(&a.rep_s)));
        PHASE(stage(c->rst_rep_e, rep_e, (size_t)n_rep, 4, reinterpret_cast<const void **>(&a.rep_e)));
    }
    return rst_run(c, a);
}

} // extern "C"
