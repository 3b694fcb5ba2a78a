// filter_lib.hip -- libraft_hip_flt.so: raft_hip_filter_overlaps_device / _host (include/raft_hip_flt.h), the kept records of a stream.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this call needs nothing of the engine but the context it is handed -- the stream, and
// buffers registered with the context like every other (fl_*, and the queries' shared staging q_col).  It reads no finished pass and
// leaves the context's state as it is.
#include "query_host.hpp"
#include "../../include/raft_hip_flt.h"
#include "filter.hpp"

#include <algorithm>

namespace {

struct FltCall {
    RecordCols rec;
    const int32_t *matches, *block;
    int32_t permille, min_span;
    int32_t *out[6];
    raft_hip_flt_summary *sum; double *kernel_seconds;
};

constexpr const char *kWho = "filter_overlaps";

// what both forms check before anything is staged
int check_call(raft_hip_ctx *c, const FltCall &a)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (a.permille < 0 || a.permille > 1000) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "min_identity_permille outside [0, 1000]");
    if (a.min_span < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "min_span is negative");
    if (a.rec.n_rec < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "n_rec is negative");
    if (a.rec.n_rec == 0) return RAFT_HIP_OK;
    for (int k = 0; k < 6; ++k)
        if (!a.rec.col[k] || !a.out[k]) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "a missing input or output column");
    if (a.permille > 0 && (!a.matches || !a.block)) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "min_identity_permille > 0 needs matches and block");
    return RAFT_HIP_OK;
}

// the device form's outputs: no range [out, out + n_rec) may meet an input column or another output
int check_ranges(raft_hip_ctx *c, const FltCall &a)
{
    const uintptr_t bytes = (uintptr_t)a.rec.n_rec * 4;
    const auto meet = [bytes](const void *x, const void *y) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(x), q = reinterpret_cast<uintptr_t>(y);
        return x && y && p < q + bytes && q < p + bytes;
    };
    for (int k = 0; k < 6 && bytes; ++k) {
        for (int j = 0; j < 6; ++j)
            if (meet(a.out[k], a.rec.col[j]) || (j != k && meet(a.out[k], a.out[j]))) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "an output column overlaps an input or another output");
        if (meet(a.out[k], a.matches) || meet(a.out[k], a.block)) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "an output column overlaps an input or another output");
    }
    return RAFT_HIP_OK;
}

// a: device arrays all.  back: the host form's destinations (the kept columns are then copied there from a.out), or NULL.
int flt_run(raft_hip_ctx *c, const FltCall &a, int32_t *const *back)
{
    const int64_t n_rec = a.rec.n_rec;
    raft_hip_flt_summary s{n_rec, 0, 0, 0, -1, 0};
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    if (n_rec > 0) {
        const long long n_tiles = flt_tiles(n_rec);
        const int scan_nb = std::max(scan_blocks(n_tiles), 1);
        HIP_TRY(c, c->fl_bits.ensure((size_t)n_tiles * kFltTileWords * 8));
        HIP_TRY(c, c->fl_tile_cnt.ensure((size_t)n_tiles * 4));
        HIP_TRY(c, c->fl_tile_base.ensure(((size_t)n_tiles + 1) * 8));
        HIP_TRY(c, c->fl_scan.ensure(((size_t)scan_nb + 1) * 8));
        HIP_TRY(c, c->fl_ctl.ensure((size_t)kFltCtlWords * 8));
        QueryTimer timer(c, a.kernel_seconds);
        unsigned long long *ctl = c->fl_ctl.as<unsigned long long>();
        const int32_t *const *col = a.rec.col;
        PHASE(timer.start());
        PHASE(clear_ctl(c, ctl, kFltCtlWords));
        const bool ident = a.permille > 0;
        const FltFlagArgs F{col[1], col[2], col[4], col[5], ident ? a.matches : nullptr, ident ? a.block : nullptr, (long long)n_rec, n_tiles,
                            a.permille, a.min_span, c->fl_bits.as<unsigned long long>(), c->fl_tile_cnt.as<int32_t>(), ctl};
        const bool vec = ident ? aligned16(a.rec, a.matches, a.block) : aligned16(a.rec);
        const dim3 grid(flt_grid(n_tiles)), block(kFltThreads);
        if (vec && ident) hipLaunchKernelGGL((flt_flag_kernel<true, true>), grid, block, 0, c->stream, F);
        else if (vec) hipLaunchKernelGGL((flt_flag_kernel<true, false>), grid, block, 0, c->stream, F);
        else if (ident) hipLaunchKernelGGL((flt_flag_kernel<false, true>), grid, block, 0, c->stream, F);
        else hipLaunchKernelGGL((flt_flag_kernel<false, false>), grid, block, 0, c->stream, F);
        long long *tile_base = c->fl_tile_base.as<long long>();
        exclusive_scan<FltTileCount, 1>(c->stream, FltTileCount{c->fl_tile_cnt.as<int32_t>()}, n_tiles, c->fl_scan.as<long long>(), ScanOut<1>{{tile_base}});
        const FltScatterArgs S{{col[0], col[1], col[2], col[3], col[4], col[5]}, {a.out[0], a.out[1], a.out[2], a.out[3], a.out[4], a.out[5]},
                               (long long)n_rec, n_tiles, c->fl_bits.as<unsigned long long>(), tile_base, ctl};
        if (aligned16(a.rec)) hipLaunchKernelGGL(flt_scatter_kernel<true>, grid, block, 0, c->stream, S);
        else hipLaunchKernelGGL(flt_scatter_kernel<false>, grid, block, 0, c->stream, S);
        HIP_TRY(c, hipGetLastError());
        PHASE(timer.stop());
        unsigned long long h_ctl[kFltCtlWords] = {};
        long long n_kept = 0;
        PHASE(read_ctl(c, ctl, h_ctl, kFltCtlWords));
        PHASE(queue_copies(c, {{&n_kept, tile_base + n_tiles, 8}}));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        PHASE(timer.seconds(a.kernel_seconds));
        if (n_kept < 0 || n_kept > n_rec) { c->last_error = "filter_overlaps: the kept count is outside [0, n_rec]"; return RAFT_HIP_ERR_DEVICE; }
        if (back) {
            for (int k = 0; k < 6; ++k) PHASE(queue_copies(c, {{back[k], a.out[k], (size_t)n_kept * 4}}));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        s.n_kept = n_kept;
        s.below_identity = (int64_t)h_ctl[kFltBelowIdentity]; s.below_span = (int64_t)h_ctl[kFltBelowSpan];
        s.first_kept = h_ctl[kFltFirst] == ~0ull ? -1 : (int64_t)h_ctl[kFltFirst];
        s.symmetric = h_ctl[kFltSymmetric] ? 1 : 0;
    }
    if (a.sum) *a.sum = s;
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_flt_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_filter_overlaps_device(raft_hip_ctx *c, int64_t n_rec, const int32_t *d_qid, const int32_t *d_qs, const int32_t *d_qe,
                                    const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te, const int32_t *d_matches,
                                    const int32_t *d_block, int32_t min_identity_permille, int32_t min_span,
                                    int32_t *d_out_qid, int32_t *d_out_qs, int32_t *d_out_qe, int32_t *d_out_tid, int32_t *d_out_ts,
                                    int32_t *d_out_te, raft_hip_flt_summary *sum, double *kernel_seconds)
{
    const FltCall a{{n_rec, {d_qid, d_qs, d_qe, d_tid, d_ts, d_te}}, d_matches, d_block, min_identity_permille, min_span,
                    {d_out_qid, d_out_qs, d_out_qe, d_out_tid, d_out_ts, d_out_te}, sum, kernel_seconds};
    PHASE(check_call(c, a));
    PHASE(check_ranges(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return flt_run(c, a, nullptr);
}

// The same from host arrays: the six columns staged through q_col, which no pass uses, the two quality columns through fl_quality; the
// kept columns go into fl_out and from there, n_kept values each, to the caller -- who may have given the input arrays themselves.
int raft_hip_filter_overlaps_host(raft_hip_ctx *c, int64_t n_rec, const int32_t *qid, const int32_t *qs, const int32_t *qe,
                                  const int32_t *tid, const int32_t *ts, const int32_t *te, const int32_t *matches,
                                  const int32_t *block, int32_t min_identity_permille, int32_t min_span,
                                  int32_t *out_qid, int32_t *out_qs, int32_t *out_qe, int32_t *out_tid, int32_t *out_ts,
                                  int32_t *out_te, raft_hip_flt_summary *sum, double *kernel_seconds)
{
    FltCall a{{n_rec, {qid, qs, qe, tid, ts, te}}, matches, block, min_identity_permille, min_span,
              {out_qid, out_qs, out_qe, out_tid, out_ts, out_te}, sum, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    int32_t *const back[6] = {out_qid, out_qs, out_qe, out_tid, out_ts, out_te};
    if (n_rec > 0) {
        PHASE(stage_columns(c, c->q_col, a.rec));
        if (min_identity_permille > 0) {
            PHASE(stage_host(c, c->fl_quality[0], matches, (size_t)n_rec, &a.matches));
            PHASE(stage_host(c, c->fl_quality[1], block, (size_t)n_rec, &a.block));
        }
        for (int k = 0; k < 6; ++k) {
            HIP_TRY(c, c->fl_out[k].ensure((size_t)n_rec * 4));
            a.out[k] = c->fl_out[k].as<int32_t>();
        }
    }
    return flt_run(c, a, back);
}

} // extern "C"
