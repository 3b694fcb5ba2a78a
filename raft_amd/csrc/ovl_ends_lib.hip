// ovl_ends_lib.hip -- libraft_hip_end.so: raft_hip_overlap_ends_device / _host (include/raft_hip_end.h), the kind of every record of a
// stream and the ends of every read the records support.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this call needs nothing of the engine but the context it is handed -- the stream, and
// buffers registered with the context like every other (en_*, and the queries' shared staging q_len, q_col).  It reads no finished
// pass and leaves the context's state as it is.
#include "query_host.hpp"
#include "../../include/raft_hip_end.h"
#include "ovl_ends.hpp"

namespace {

struct EndCall {
    int32_t n_reads;
    const int32_t *len;
    RecordCols rec;
    const uint8_t *strand;
    int32_t max_overhang, min_ratio, symmetric;
    int32_t *counts; uint8_t *status, *kinds;
    raft_hip_end_summary *sum; int64_t *error_index; double *kernel_seconds;
};

constexpr const char *kWho = "overlap_ends";

// what both forms check before anything is staged
int check_call(raft_hip_ctx *c, const EndCall &a)
{
    return check_ends_rule_call(c, kWho, a.max_overhang, a.min_ratio, a.n_reads, a.len, a.rec, a.strand);
}

// the four-record loads and stores: the six columns on 16-byte lines, strand and kinds (where given) on 4-byte ones
bool vector_path(const EndCall &a)
{
    return aligned16(a.rec) && ((reinterpret_cast<uintptr_t>(a.strand) | reinterpret_cast<uintptr_t>(a.kinds)) & 3) == 0;
}

// a: device arrays but for counts, status and the rest of the outputs.  kinds_back: the host form's destination of the kind bytes
// (copied there from a.kinds once the stream is known to be clean), or NULL.
int end_run(raft_hip_ctx *c, const EndCall &a, uint8_t *kinds_back)
{
    const int64_t n_rec = a.rec.n_rec;
    const size_t n = (size_t)std::max(a.n_reads, 1);
    HIP_TRY(c, c->en_cnt.ensure(n * kEndCounts * 4));
    HIP_TRY(c, c->en_status.ensure(n));
    HIP_TRY(c, c->en_ctl.ensure((size_t)kEndsCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    unsigned long long *ctl = c->en_ctl.as<unsigned long long>();
    HIP_TRY(c, hipMemsetAsync(c->en_cnt.p, 0, n * kEndCounts * 4, c->stream));
    PHASE(clear_ctl(c, ctl, kEndsCtlWords));
    PHASE(timer.start());
    if (n_rec > 0) {
        const int32_t *const *col = a.rec.col;
        const EndsArgs A{a.len, col[0], col[1], col[2], col[3], col[4], col[5], a.strand, a.kinds, (long long)n_rec, a.n_reads,
                         a.max_overhang, a.min_ratio, a.symmetric ? 1 : 0, c->en_cnt.as<unsigned>(), ctl};
        const dim3 grid(stream_grid(n_rec)), block(kStreamThreads);
        if (vector_path(a)) hipLaunchKernelGGL(ends_kernel<true>, grid, block, 0, c->stream, A);
        else hipLaunchKernelGGL(ends_kernel<false>, grid, block, 0, c->stream, A);
    }
    if (a.n_reads > 0)
        hipLaunchKernelGGL(ends_status_kernel, dim3(grid_for(a.n_reads, 256, 1024)), dim3(256), 0, c->stream, c->en_cnt.as<unsigned>(), a.n_reads,
                           c->en_status.as<uint8_t>(), ctl);
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kEndsCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kEndsCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(a.kernel_seconds));
    PHASE(first_bad_record(c, h_ctl[0], a.error_index, "overlap_ends: a record names a read id outside [0, n_reads)"));
    PHASE(queue_copies(c, {{a.counts, c->en_cnt.p, (size_t)a.n_reads * kEndCounts * 4}, {a.status, c->en_status.p, (size_t)a.n_reads},
                           {kinds_back, a.kinds, (size_t)n_rec}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum) {
        const unsigned long long *k = h_ctl + kEndsCtlKinds, *s = h_ctl + kEndsCtlStatus;
        *a.sum = raft_hip_end_summary{n_rec, (int64_t)k[0], (int64_t)k[1], (int64_t)k[2], (int64_t)k[3], (int64_t)k[4], (int64_t)k[5], (int64_t)k[6],
                                      (int64_t)s[0], (int64_t)s[1], (int64_t)s[2], (int64_t)s[3], (int64_t)s[4]};
    }
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_end_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_overlap_ends_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                                 const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                 const uint8_t *d_strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t symmetric,
                                 int32_t *counts, uint8_t *status, uint8_t *d_kinds, raft_hip_end_summary *sum, int64_t *error_index,
                                 double *kernel_seconds)
{
    const EndCall a{n_reads, d_read_len, {n_rec, {d_qid, d_qs, d_qe, d_tid, d_ts, d_te}}, d_strand, max_overhang, min_ratio_permille, symmetric,
                    counts, status, d_kinds, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return end_run(c, a, nullptr);
}

// The same from host arrays: the lengths and the six columns staged through q_len and q_col, which no pass uses, the strand bytes
// through en_strand; the kind bytes are written to en_kinds and go to the caller from there.
int raft_hip_overlap_ends_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                               const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                               const uint8_t *strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t symmetric,
                               int32_t *counts, uint8_t *status, uint8_t *kinds, raft_hip_end_summary *sum, int64_t *error_index,
                               double *kernel_seconds)
{
    EndCall a{n_reads, read_len, {n_rec, {qid, qs, qe, tid, ts, te}}, strand, max_overhang, min_ratio_permille, symmetric,
              counts, status, kinds, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
    if (n_rec > 0) {
        PHASE(stage_columns(c, c->q_col, a.rec));
        PHASE(stage_host(c, c->en_strand, strand, (size_t)n_rec, &a.strand));
        if (kinds) {
            HIP_TRY(c, c->en_kinds.ensure((size_t)n_rec));
            a.kinds = c->en_kinds.as<uint8_t>();
        }
    }
    return end_run(c, a, kinds);
}

} // extern "C"
