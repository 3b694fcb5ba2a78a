// lift_lib.hip -- libraft_hip_lift.so: raft_hip_lift_overlaps_device / _host (include/raft_hip_lift.h), the record stream lifted onto
// the fragment table.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this call needs nothing of the engine but the context it is handed -- the fragment rows
// a finished pass left (engine_ctx.hpp), the stream, and buffers registered with the context like every other (lf_*, and the
// queries' shared staging q_col, q_csr_a).  Nothing of a pass is written.
#include "query_host.hpp"
#include "../../include/raft_hip_lift.h"
#include "lift.hpp"

#include <algorithm>

namespace {

struct LiftCall {
    int32_t n_reads; RecordCols rec; const uint8_t *strand;
    CsrArg table;                                                             // device arrays, or all NULL with count -1: the context's pass
    int32_t min_len; int64_t out_cap;
    void *out[8];                                                             // qfrag, qs, qe, tfrag, ts, te (int32), rev (uint8), src (int32)
    raft_hip_lift_summary *sum; int64_t *error_index; double *kernel_seconds;
};

constexpr const char *kWho = "lift_overlaps";
constexpr size_t kOutBytes[8] = {4, 4, 4, 4, 4, 4, 1, 4};
constexpr const char *kTooMany = "too many records, rows or outputs";

// what both forms check before anything is staged: counts, columns, the table, the state an own-pass call needs
int check_call(raft_hip_ctx *c, const LiftCall &a)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (a.n_reads < 0 || a.rec.n_rec < 0 || a.out_cap < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "a negative count");
    if (a.min_len < 1) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "min_len is below 1");
    if (a.rec.n_rec > 0 && (!record_cols_ok(a.rec, false, TargetCols::always) || !a.strand))
        return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "a missing column (the six and strand)");
    const CsrKind table = csr_arg_kind(a.table);
    if (table == CsrKind::bad || table == CsrKind::none) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, kBadArgs);
    if (a.rec.n_rec >= (int64_t(1) << 30) || a.table.count >= (int64_t(1) << 31) - 1) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, kTooMany);
    if (table == CsrKind::own) {                              // the context's own finished pass
        if (!c->finished || c->pending_err) return refuse(c, RAFT_HIP_ERR_STATE, kWho, kNoPass);
        if (a.n_reads != c->sum.n_reads) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, kOtherReads);
        if (c->sum.n_fragments >= (int64_t(1) << 31) - 1) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, kTooMany);
    }
    return RAFT_HIP_OK;
}

bool vector_path(const LiftCall &a)
{
    return aligned16(a.rec) && (reinterpret_cast<uintptr_t>(a.strand) & 3) == 0;
}

// a: device arrays all but the outputs, which are the caller's: device arrays (host == false) or host arrays, then filled through lf_out.
int lift_run(raft_hip_ctx *c, const LiftCall &a, bool host)
{
    const bool own_table = a.table.count == -1;
    const CsrDev table = resolve_csr(a.table, c->frag_off, c->frag_begin, c->frag_end, c->sum.n_fragments);
    const long long n_frag = table.count;
    const int64_t n_rec = a.rec.n_rec;
    const long long n_tiles = lift_tiles(n_rec);
    const int scan_nb = std::max(scan_blocks(n_tiles), 1);
    const size_t n = (size_t)std::max(a.n_reads, 1), nt = (size_t)std::max<long long>(n_tiles, 1);
    HIP_TRY(c, c->lf_digest.ensure(n * sizeof(FragDigest)));
    HIP_TRY(c, c->lf_tile_cnt.ensure(nt * 8));
    HIP_TRY(c, c->lf_lane_cnt.ensure(nt * kStreamThreads * 4));
    HIP_TRY(c, c->lf_tile_base.ensure((nt + 1) * 8));
    HIP_TRY(c, c->lf_scan.ensure(((size_t)scan_nb + 1) * 8));
    HIP_TRY(c, c->lf_ctl.ensure((size_t)kLiftCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    double head_seconds = 0.0, tail_seconds = 0.0;            // (two spans: the host reads n_out in between)
    unsigned long long *ctl = c->lf_ctl.as<unsigned long long>();
    long long *tile_base = c->lf_tile_base.as<long long>();
    const int32_t *const *col = a.rec.col;
    LiftArgs A{col[0], col[1], col[2], col[3], col[4], col[5], a.strand, (long long)n_rec, n_tiles, a.n_reads, a.min_len, table.x, table.y,
               c->lf_digest.as<FragDigest>(), ctl, c->lf_tile_cnt.as<long long>(), c->lf_lane_cnt.as<int32_t>(), tile_base, 0,
               {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr};
    const dim3 grid(lift_grid(n_tiles)), block(kStreamThreads);
    const bool vec = vector_path(a);
    PHASE(timer.start());
    PHASE(clear_ctl(c, ctl, kLiftCtlWords));
    if (a.n_reads > 0 || !own_table)
        hipLaunchKernelGGL(frag_digest_kernel, dim3((unsigned)(((long long)a.n_reads + 1 + 255) / 256)), dim3(256), 0, c->stream, table.off, table.x, table.y,
                           a.n_reads, n_frag, c->lf_digest.as<FragDigest>(), ctl);
    long long n_out = 0;
    if (n_rec > 0) {
        if (vec) hipLaunchKernelGGL(lift_count_kernel<true>, grid, block, 0, c->stream, A);
        else hipLaunchKernelGGL(lift_count_kernel<false>, grid, block, 0, c->stream, A);
        exclusive_scan<LiftTileCount, 1>(c->stream, LiftTileCount{c->lf_tile_cnt.as<long long>()}, n_tiles, c->lf_scan.as<long long>(), ScanOut<1>{{tile_base}});
    }
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kLiftCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kLiftCtlWords));
    // (a broken table: the count kernel left at once and tile_cnt holds nothing; n_out is then not looked at)
    if (n_rec > 0) PHASE(queue_copies(c, {{&n_out, tile_base + n_tiles, 8}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // (the one wait: n_out sizes the outputs)
    PHASE(timer.seconds(&head_seconds));
    if (a.kernel_seconds) *a.kernel_seconds = head_seconds;
    if (h_ctl[kLiftBadTable]) {
        c->last_error = "lift_overlaps: frag_offset does not begin at 0, ascend and end at n_frag, or a read's rows descend or are not 0 <= begin <= end";
        return RAFT_HIP_ERR_PARAM;
    }
    PHASE(first_bad_record(c, h_ctl[kLiftFirstBad], a.error_index, "lift_overlaps: a record names a read id outside [0, n_reads)"));
    if (n_out < 0) { c->last_error = "lift_overlaps: the output count is negative"; return RAFT_HIP_ERR_DEVICE; }
    if (n_out >= (int64_t(1) << 31) - 1) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, kTooMany);
    if (a.sum)
        *a.sum = raft_hip_lift_summary{n_rec, n_out, (int64_t)h_ctl[kLiftNone], (int64_t)h_ctl[kLiftCut], (int64_t)h_ctl[kLiftDropped], (int64_t)h_ctl[kLiftMost]};
    bool any = false;
    for (int k = 0; k < 8; ++k) any = any || a.out[k];
    if (!any) return RAFT_HIP_OK;                             // the size query
    if (n_out > a.out_cap) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, "out_cap is below the summary's n_out");
    if (n_out == 0) return RAFT_HIP_OK;
    void *dev[8];
    for (int k = 0; k < 8; ++k) {
        dev[k] = a.out[k];
        if (host && a.out[k]) {
            HIP_TRY(c, c->lf_out[k].ensure((size_t)n_out * kOutBytes[k]));
            dev[k] = c->lf_out[k].p;
        }
    }
    for (int k = 0; k < 6; ++k) A.out[k] = static_cast<int32_t *>(dev[k]);
    A.rev = static_cast<uint8_t *>(dev[6]); A.src = static_cast<int32_t *>(dev[7]);
    A.n_out = n_out;
    PHASE(timer.start());
    if (vec) hipLaunchKernelGGL(lift_fill_kernel<true>, grid, block, 0, c->stream, A);
    else hipLaunchKernelGGL(lift_fill_kernel<false>, grid, block, 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    if (host)
        for (int k = 0; k < 8; ++k) PHASE(queue_copies(c, {{a.out[k], dev[k], (size_t)n_out * kOutBytes[k]}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(&tail_seconds));
    if (a.kernel_seconds) *a.kernel_seconds = head_seconds + tail_seconds;
    return RAFT_HIP_OK;
}

LiftCall make_call(int32_t n_reads, const raft_hip_records *rec, const uint8_t *strand, const raft_hip_frag_table *table, int32_t min_len, int64_t out_cap,
                   int32_t *qfrag, int32_t *qs, int32_t *qe, int32_t *tfrag, int32_t *ts, int32_t *te, uint8_t *rev, int32_t *src,
                   raft_hip_lift_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    return LiftCall{n_reads, {rec->n_rec, {rec->d_qid, rec->d_qs, rec->d_qe, rec->d_tid, rec->d_ts, rec->d_te}}, strand,
                    {table->n_frag, table->frag_offset, table->frag_begin, table->frag_end}, min_len, out_cap,
                    {qfrag, qs, qe, tfrag, ts, te, rev, src}, sum, error_index, kernel_seconds};
}

} // namespace

extern "C" {

int raft_hip_lift_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_lift_overlaps_device(raft_hip_ctx *c, int32_t n_reads, const raft_hip_records *records, const uint8_t *d_strand,
                                  const raft_hip_frag_table *table, int32_t min_len, int64_t out_cap, int32_t *d_qfrag, int32_t *d_qs,
                                  int32_t *d_qe, int32_t *d_tfrag, int32_t *d_ts, int32_t *d_te, uint8_t *d_rev, int32_t *d_src,
                                  raft_hip_lift_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    if (!records || !table) return RAFT_HIP_ERR_PARAM;
    const LiftCall a = make_call(n_reads, records, d_strand, table, min_len, out_cap, d_qfrag, d_qs, d_qe, d_tfrag, d_ts, d_te, d_rev, d_src, sum,
                                 error_index, kernel_seconds);
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return lift_run(c, a, false);
}

// The same from host arrays: the six columns staged through q_col and a table the caller gave through q_csr_a, which no pass uses, the
// strand bytes through lf_strand; the outputs are written to lf_out and go to the caller from there.
int raft_hip_lift_overlaps_host(raft_hip_ctx *c, int32_t n_reads, const raft_hip_records *records, const uint8_t *strand,
                                const raft_hip_frag_table *table, int32_t min_len, int64_t out_cap, int32_t *qfrag, int32_t *qs,
                                int32_t *qe, int32_t *tfrag, int32_t *ts, int32_t *te, uint8_t *rev, int32_t *src,
                                raft_hip_lift_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    if (!records || !table) return RAFT_HIP_ERR_PARAM;
    LiftCall a = make_call(n_reads, records, strand, table, min_len, out_cap, qfrag, qs, qe, tfrag, ts, te, rev, src, sum, error_index, kernel_seconds);
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    if (a.rec.n_rec > 0) {
        PHASE(stage_columns(c, c->q_col, a.rec));
        PHASE(stage_host(c, c->lf_strand, strand, (size_t)a.rec.n_rec, &a.strand));
    }
    if (csr_arg_kind(a.table) == CsrKind::given) PHASE(stage_csr(c, c->q_csr_a, a.table, n_reads));
    return lift_run(c, a, true);
}

} // extern "C"
