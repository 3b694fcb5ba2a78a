// best_ovl_lib.hip -- libraft_hip_best.so: raft_hip_best_overlaps_device / _host (include/raft_hip_best.h), the best overlap of every
// read end and whether it is mutual.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this call needs nothing of the engine but the context it is handed -- the stream, and
// buffers registered with the context like every other (bo_*, and the queries' shared staging q_len, q_col).  It reads no finished
// pass and leaves the context's state as it is.
#include "query_host.hpp"
#include "../../include/raft_hip_best.h"
#include "best_ovl.hpp"

namespace {

struct BestCall {
    int32_t n_reads;
    const int32_t *len;
    RecordCols rec;
    const uint8_t *strand, *skip;
    int32_t max_overhang, min_ratio, symmetric;
    int32_t *partner, *span; uint8_t *flags;
    raft_hip_best_summary *sum; int64_t *error_index; double *kernel_seconds;
};

constexpr const char *kWho = "best_overlaps";

// what both forms check before anything is staged
int check_call(raft_hip_ctx *c, const BestCall &a)
{
    return check_ends_rule_call(c, kWho, a.max_overhang, a.min_ratio, a.n_reads, a.len, a.rec, a.strand);
}

// the four-record loads: the six columns on 16-byte lines, strand on a 4-byte one
bool vector_path(const BestCall &a) { return aligned16(a.rec) && (reinterpret_cast<uintptr_t>(a.strand) & 3) == 0; }

// a: device arrays but for partner, span, flags and the rest of the outputs
int best_run(raft_hip_ctx *c, const BestCall &a)
{
    const int64_t n_rec = a.rec.n_rec;
    const size_t n = (size_t)std::max(a.n_reads, 1);
    HIP_TRY(c, c->bo_dig.ensure(n * 4));
    HIP_TRY(c, c->bo_tab.ensure(n * 2 * 8));
    HIP_TRY(c, c->bo_partner.ensure(n * 2 * 4));
    HIP_TRY(c, c->bo_span.ensure(n * 2 * 4));
    HIP_TRY(c, c->bo_flags.ensure(n));
    HIP_TRY(c, c->bo_ctl.ensure((size_t)kBestCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    unsigned long long *ctl = c->bo_ctl.as<unsigned long long>(), *tab = c->bo_tab.as<unsigned long long>();
    PHASE(clear_ctl(c, ctl, kBestCtlWords));
    PHASE(timer.start());
    HIP_TRY(c, hipMemsetAsync(tab, 0, n * 2 * 8, c->stream));
    if (a.n_reads > 0)
        hipLaunchKernelGGL(best_digest_kernel, dim3(grid_for(a.n_reads, 256, 1024)), dim3(256), 0, c->stream, a.len, a.skip, a.n_reads,
                           c->bo_dig.as<unsigned>());
    if (n_rec > 0) {
        const int32_t *const *col = a.rec.col;
        const BestArgs A{c->bo_dig.as<unsigned>(), col[0], col[1], col[2], col[3], col[4], col[5], a.strand, (long long)n_rec, a.n_reads,
                         a.max_overhang, a.min_ratio, a.symmetric ? 1 : 0, tab, ctl};
        const dim3 grid(stream_grid(n_rec)), block(kStreamThreads);
        if (vector_path(a)) hipLaunchKernelGGL(best_kernel<true>, grid, block, 0, c->stream, A);
        else hipLaunchKernelGGL(best_kernel<false>, grid, block, 0, c->stream, A);
    }
    if (a.n_reads > 0)
        hipLaunchKernelGGL(best_pairs_kernel, dim3(grid_for(a.n_reads, 256, 1024)), dim3(256), 0, c->stream, tab, c->bo_dig.as<unsigned>(), a.n_reads,
                           c->bo_partner.as<int32_t>(), c->bo_span.as<int32_t>(), c->bo_flags.as<uint8_t>(), ctl);
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kBestCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kBestCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(a.kernel_seconds));
    PHASE(first_bad_record(c, h_ctl[0], a.error_index, "best_overlaps: a record names a read id outside [0, n_reads)"));
    PHASE(queue_copies(c, {{a.partner, c->bo_partner.p, (size_t)a.n_reads * 2 * 4}, {a.span, c->bo_span.p, (size_t)a.n_reads * 2 * 4},
                           {a.flags, c->bo_flags.p, (size_t)a.n_reads}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum) {
        const unsigned long long *v = h_ctl + kBestCtlViews, *r = h_ctl + kBestCtlReads;
        *a.sum = raft_hip_best_summary{n_rec, (int64_t)v[0], (int64_t)v[1], (int64_t)r[0], (int64_t)r[1], (int64_t)r[2], (int64_t)r[3],
                                       (int64_t)r[4], (int64_t)r[5]};
    }
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_best_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_best_overlaps_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                                  const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                  const uint8_t *d_strand, const uint8_t *d_skip, int32_t max_overhang, int32_t min_ratio_permille,
                                  int32_t symmetric, int32_t *partner, int32_t *span, uint8_t *flags, raft_hip_best_summary *sum,
                                  int64_t *error_index, double *kernel_seconds)
{
    const BestCall a{n_reads, d_read_len, {n_rec, {d_qid, d_qs, d_qe, d_tid, d_ts, d_te}}, d_strand, d_skip, max_overhang, min_ratio_permille,
                     symmetric, partner, span, flags, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return best_run(c, a);
}

// The same from host arrays: the lengths and the six columns staged through q_len and q_col, which no pass uses, the strand bytes
// through bo_strand and the skip bytes, where given, through bo_skip.
int raft_hip_best_overlaps_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                                const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                                const uint8_t *strand, const uint8_t *skip, int32_t max_overhang, int32_t min_ratio_permille,
                                int32_t symmetric, int32_t *partner, int32_t *span, uint8_t *flags, raft_hip_best_summary *sum,
                                int64_t *error_index, double *kernel_seconds)
{
    BestCall a{n_reads, read_len, {n_rec, {qid, qs, qe, tid, ts, te}}, strand, skip, max_overhang, min_ratio_permille,
               symmetric, partner, span, flags, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
    if (skip && n_reads > 0) PHASE(stage_host(c, c->bo_skip, skip, (size_t)n_reads, &a.skip));
    if (n_rec > 0) {
        PHASE(stage_columns(c, c->q_col, a.rec));
        PHASE(stage_host(c, c->bo_strand, strand, (size_t)n_rec, &a.strand));
    }
    return best_run(c, a);
}

} // extern "C"
