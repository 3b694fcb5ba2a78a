// repeat_stats_lib.hip -- libraft_hip_rst.so: raft_hip_repeat_stats_device / _host (include/raft_hip_rst.h), one row per repeat run.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this query needs nothing of the engine but the context it is handed -- the coverage and
// the repeat arrays a finished pass left (engine_ctx.hpp), the stream, and buffers registered with the context like every other
// (rst_*, and the queries' shared staging and decoded coverage q_*).
#include "cov_decode.hpp"
#include "../../include/raft_hip_rst.h"
#include "repeat_stats.hpp"

#include <algorithm>

static_assert(kRstEmpty == RAFT_HIP_RST_EMPTY && kRstAtStart == RAFT_HIP_RST_AT_START && kRstAtEnd == RAFT_HIP_RST_AT_END, "the kernels write the header's bits");

namespace {

struct RstCall {
    int32_t n_reads; const int32_t *len; RecordCols rec;
    int32_t symmetric;
    CsrArg rep;                                                               // device arrays, or all NULL with count -1: the context's pass
    int32_t threshold;
    int32_t *cnt[3];                                                          // touch, span, inside
    int32_t *win[4];                                                          // windows, min, max, high
    int64_t *cov_sum; uint8_t *flags;
    raft_hip_rst_summary *sum; int64_t *error_index; double *kernel_seconds;
};

// what both forms check before anything is staged: counts, columns, the three repeat arrays, the state the call needs
int check_call(raft_hip_ctx *c, const RstCall &a)
{
    const char *who = "repeat_stats";
    if (!c || a.n_reads < 0 || a.rec.n_rec < 0 || a.threshold < 0 || (a.n_reads > 0 && !a.len)) return refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);
    if (!record_cols_ok(a.rec, a.symmetric != 0, TargetCols::unless_symmetric)) return refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);
    if (a.threshold == 0 && (a.win[0] || a.win[1] || a.win[2] || a.win[3] || a.cov_sum)) return refuse(c, RAFT_HIP_ERR_PARAM, who, "threshold 0 takes no coverage output");
    const CsrKind rep = csr_arg_kind(a.rep);
    const bool own = rep == CsrKind::own;
    if (!own && rep != CsrKind::given) return refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);
    if (a.rec.n_rec >= (int64_t(1) << 30) || a.rep.count >= (int64_t(1) << 31) - 1) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, who, "too many records or runs");
    if (own || a.threshold >= 1) {                            // the context's own finished pass: its annotation, its coverage
        if (!c->finished || c->pending_err) return refuse(c, RAFT_HIP_ERR_STATE, who, kNoPass);
        if (a.n_reads != c->sum.n_reads) return refuse(c, RAFT_HIP_ERR_PARAM, who, kOtherReads);
        if (own && c->sum.n_repeats >= (int64_t(1) << 31) - 1) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, who, "too many records or runs");
    }
    return RAFT_HIP_OK;
}

int rst_run(raft_hip_ctx *c, const RstCall &a)
{
    const bool own = a.rep.count == -1, with_cov = a.threshold >= 1;
    const CsrDev rep = resolve_csr(a.rep, c->rep_off, c->rep_s, c->rep_e, c->sum.n_repeats);
    const long long n_rep = rep.count;
    const int64_t n_rec = a.rec.n_rec;
    const int32_t *const *col = a.rec.col;
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
    QueryTimer timer(c, a.kernel_seconds);
    unsigned long long *ctl = c->rst_ctl.as<unsigned long long>();
    int32_t *run_read = c->rst_run_read.as<int32_t>();
    RstSlot *slot = c->rst_slot.as<RstSlot>();
    PHASE(timer.start());
    HIP_TRY(c, hipMemsetAsync(slot, 0, nr * sizeof(RstSlot), c->stream));
    PHASE(clear_ctl(c, ctl, kRstCtlWords));
    const int32_t *cov = nullptr;
    if (with_cov) {
        if (!c->cov_valid && pass_holds_codes(c) && c->n_exc > c->exc_cap) { c->last_error = "repeat_stats: the pass's exception list is incomplete"; return RAFT_HIP_ERR_DEVICE; }
        PHASE(query_cov(c, "repeat_stats", &cov));
    }
    if (a.n_reads > 0 || !own)
        hipLaunchKernelGGL(rst_digest_kernel, dim3((unsigned)(((long long)a.n_reads + 1 + 255) / 256)), dim3(256), 0, c->stream, rep.off, rep.x, rep.y,
                           a.n_reads, n_rep, c->rst_digest.as<RstDigest>(), run_read, ctl);
    if (n_rec > 0) {                                          // (without a run too: the ids are checked)
        RstArgs A{col[0], col[1], col[2], col[3], col[4], col[5], (long long)n_rec, a.n_reads, a.symmetric ? 1 : 0,
                  rep.x, rep.y, c->rst_digest.as<RstDigest>(), slot, ctl};
        if (aligned16(a.rec)) hipLaunchKernelGGL(rst_side_kernel<true>, dim3(stream_grid(n_rec)), dim3(kStreamThreads), 0, c->stream, A);
        else hipLaunchKernelGGL(rst_side_kernel<false>, dim3(stream_grid(n_rec)), dim3(kStreamThreads), 0, c->stream, A);
    }
    RstCovOut co{c->rst_win[0].as<int32_t>(), c->rst_win[1].as<int32_t>(), c->rst_win[2].as<int32_t>(), c->rst_win[3].as<int32_t>(), c->rst_sum.as<long long>()};
    if (n_rep > 0) {
        if (with_cov)
            hipLaunchKernelGGL(rst_cov_kernel, dim3(rst_cov_grid(n_rep)), dim3(kRstCovThreads), 0, c->stream, cov, c->cov_off.as<long long>(), rep.x, rep.y,
                               run_read, n_rep, c->prm.reso, a.threshold, ctl, co);
        RstRunsArgs R{slot, rep.x, rep.y, run_read, a.len, n_rep, with_cov ? co.windows : nullptr, co.cov_sum, c->rst_cnt[0].as<int32_t>(),
                      c->rst_cnt[1].as<int32_t>(), c->rst_cnt[2].as<int32_t>(), c->rst_flags.as<uint8_t>(), ctl};
        hipLaunchKernelGGL(rst_runs_kernel, dim3(grid_for(n_rep, 256, 2048)), dim3(256), 0, c->stream, R);
    }
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kRstCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kRstCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(a.kernel_seconds));
    if (h_ctl[kRstBadOffsets]) {
        c->last_error = "repeat_stats: rep_offset does not begin at 0, ascend and end at n_rep";
        return RAFT_HIP_ERR_PARAM;
    }
    PHASE(first_bad_record(c, h_ctl[kRstFirstBad], a.error_index, "repeat_stats: a record names a read id outside [0, n_reads)"));
    for (int k = 0; k < 3; ++k) PHASE(queue_copies(c, {{a.cnt[k], c->rst_cnt[k].p, (size_t)n_rep * 4}}));
    PHASE(queue_copies(c, {{a.flags, c->rst_flags.p, (size_t)n_rep}}));
    if (with_cov) {
        for (int k = 0; k < 4; ++k) PHASE(queue_copies(c, {{a.win[k], c->rst_win[k].p, (size_t)n_rep * 4}}));
        PHASE(queue_copies(c, {{a.cov_sum, c->rst_sum.p, (size_t)n_rep * 8}}));
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
    RstCall a{n_reads, len, {0, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}}, symmetric, {n_rep, rep_off, rep_s, rep_e}, threshold,
              {touch, span, inside}, {windows, cov_min, cov_max, high}, cov_sum, flags, sum, error_index, kernel_seconds};
    if (rec && rec->n_rec != 0) {                            // (NULL or no records: every count is 0)
        a.rec = {rec->n_rec, {rec->d_qid, rec->d_qs, rec->d_qe, rec->d_tid, rec->d_ts, rec->d_te}};
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

// The same from host arrays, staged through buffers of the context that no pass uses (q_len, q_col, q_csr_a).
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
    PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
    PHASE(stage_columns(c, c->q_col, a.rec));
    if (n_rep != -1) PHASE(stage_csr(c, c->q_csr_a, a.rep, n_reads));
    return rst_run(c, a);
}

} // extern "C"
