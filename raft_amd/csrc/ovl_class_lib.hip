// ovl_class_lib.hip -- libraft_hip_ovl.so: raft_hip_repeat_overlaps_device / _host (include/raft_hip_ovl.h), the record stream
// classified against the repeat annotation.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this query needs nothing of the engine but the context it is handed -- the repeat arrays
// a finished pass left (engine_ctx.hpp), the stream, and buffers registered with the context like every other (oc_*, and the queries'
// shared staging q_*).
#include "query_host.hpp"
#include "../../include/raft_hip_ovl.h"
#include "ovl_class.hpp"

#include <algorithm>

namespace {

struct OvlCall {
    int32_t n_reads; const int32_t *len; RecordCols rec;
    int32_t symmetric, min_anchor;
    CsrArg rep;                                                               // device arrays, or all NULL with count -1: the context's pass
    uint8_t *cls; hipMemcpyKind cls_kind;
    int32_t *read_touch, *read_repeat; uint8_t *read_flags;
    raft_hip_ovl_summary *sum; int64_t *error_index; double *kernel_seconds;
};

// what both forms check before anything is staged: counts, columns, the three repeat arrays, the state an own-pass call needs
int check_call(raft_hip_ctx *c, const OvlCall &a)
{
    const char *who = "repeat_overlaps";
    if (c && a.min_anchor < 1) return refuse(c, RAFT_HIP_ERR_PARAM, who, "min_anchor < 1");
    if (!c || a.n_reads < 0 || a.rec.n_rec < 0 || (a.n_reads > 0 && !a.len)) return refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);
    if (!record_cols_ok(a.rec, a.symmetric != 0, TargetCols::unless_symmetric)) return refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);
    const CsrKind rep = csr_arg_kind(a.rep);
    if (rep == CsrKind::own) {                                // the context's own finished pass
        if (!c->finished || c->pending_err) return refuse(c, RAFT_HIP_ERR_STATE, who, kNoPass);
        if (a.n_reads != c->sum.n_reads) return refuse(c, RAFT_HIP_ERR_PARAM, who, kOtherReads);
        return RAFT_HIP_OK;
    }
    return rep == CsrKind::given ? RAFT_HIP_OK : refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);
}

int ovl_run(raft_hip_ctx *c, const OvlCall &a)
{
    const bool own = a.rep.count == -1;
    const CsrDev rep = resolve_csr(a.rep, c->rep_off, c->rep_s, c->rep_e, c->sum.n_repeats);
    const int64_t n_rec = a.rec.n_rec;
    const int32_t *const *col = a.rec.col;
    const size_t n = (size_t)std::max(a.n_reads, 1);
    HIP_TRY(c, c->oc_digest.ensure(n * sizeof(OvlDigest)));
    HIP_TRY(c, c->oc_touch.ensure(n * 4)); HIP_TRY(c, c->oc_repeat.ensure(n * 4)); HIP_TRY(c, c->oc_flagw.ensure(n * 4));
    HIP_TRY(c, c->oc_tally.ensure(n * 8));
    HIP_TRY(c, c->oc_flags.ensure(n));
    HIP_TRY(c, c->oc_ctl.ensure((size_t)kOvlCtlWords * 8));
    if (a.cls) HIP_TRY(c, c->oc_cls.ensure((size_t)std::max<int64_t>(n_rec, 1) + 4));
    QueryTimer timer(c, a.kernel_seconds);
    unsigned long long *ctl = c->oc_ctl.as<unsigned long long>();
    HIP_TRY(c, hipMemsetAsync(c->oc_tally.p, 0, n * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->oc_flagw.p, 0, n * 4, c->stream));
    PHASE(clear_ctl(c, ctl, kOvlCtlWords));
    PHASE(timer.start());
    if (a.n_reads > 0 || !own)
        hipLaunchKernelGGL(ovl_digest_kernel, dim3((unsigned)(((long long)a.n_reads + 1 + 255) / 256)), dim3(256), 0, c->stream, rep.off, rep.x, rep.y,
                           a.n_reads, rep.count, c->oc_digest.as<OvlDigest>(), ctl);
    if (n_rec > 0) {
        OvlArgs A{a.len, col[0], col[1], col[2], col[3], col[4], col[5], (long long)n_rec, a.n_reads, a.symmetric ? 1 : 0, a.min_anchor,
                  rep.off, rep.x, rep.y, c->oc_digest.as<OvlDigest>(), a.cls ? c->oc_cls.as<uint8_t>() : nullptr,
                  c->oc_tally.as<unsigned long long>(), c->oc_flagw.as<unsigned>(), ctl};
        if (aligned16(a.rec)) hipLaunchKernelGGL(ovl_class_kernel<true>, dim3(stream_grid(n_rec)), dim3(kStreamThreads), 0, c->stream, A);
        else hipLaunchKernelGGL(ovl_class_kernel<false>, dim3(stream_grid(n_rec)), dim3(kStreamThreads), 0, c->stream, A);
    }
    if (a.n_reads > 0)
        hipLaunchKernelGGL(ovl_reads_kernel, dim3((unsigned)std::min<long long>(((long long)a.n_reads + 255) / 256, 1024)), dim3(256), 0, c->stream,
                           c->oc_flagw.as<unsigned>(), c->oc_tally.as<unsigned long long>(), a.n_reads, c->oc_flags.as<uint8_t>(),
                           c->oc_touch.as<int32_t>(), c->oc_repeat.as<int32_t>(), ctl);
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kOvlCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kOvlCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(a.kernel_seconds));
    if (h_ctl[kOvlBadOffsets]) {
        c->last_error = "repeat_overlaps: rep_offset does not begin at 0, ascend and end at n_rep";
        return RAFT_HIP_ERR_PARAM;
    }
    PHASE(first_bad_record(c, h_ctl[kOvlFirstBad], a.error_index, "repeat_overlaps: a record names a read id outside [0, n_reads)"));
    PHASE(queue_copies(c, {{a.cls, c->oc_cls.p, (size_t)n_rec, a.cls_kind},
                           {a.read_touch, c->oc_touch.p, (size_t)a.n_reads * 4}, {a.read_repeat, c->oc_repeat.p, (size_t)a.n_reads * 4},
                           {a.read_flags, c->oc_flags.p, (size_t)a.n_reads}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum) {
        const unsigned long long *t = h_ctl + kOvlRecTotals;
        a.sum->n_records = n_rec;
        a.sum->q_touch = (int64_t)t[0]; a.sum->t_touch = (int64_t)t[1]; a.sum->q_repeat = (int64_t)t[2]; a.sum->t_repeat = (int64_t)t[3];
        a.sum->both_repeat = (int64_t)t[4]; a.sum->q_contained = (int64_t)t[5]; a.sum->t_contained = (int64_t)t[6];
        a.sum->reads_contained = (int64_t)h_ctl[kOvlReadTotals]; a.sum->reads_repeat_contained = (int64_t)h_ctl[kOvlReadTotals + 1];
    }
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_ovl_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_repeat_overlaps_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid, const int32_t *d_qs,
                                    const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te, int32_t symmetric, int32_t min_anchor,
                                    int64_t n_rep, const int64_t *d_rep_offset, const int32_t *d_rep_s, const int32_t *d_rep_e, uint8_t *d_cls,
                                    int32_t *read_touch, int32_t *read_repeat, uint8_t *read_flags, raft_hip_ovl_summary *sum, int64_t *error_index,
                                    double *kernel_seconds)
{
    const OvlCall a{n_reads, d_read_len, {n_rec, {d_qid, d_qs, d_qe, d_tid, d_ts, d_te}}, symmetric, min_anchor, {n_rep, d_rep_offset, d_rep_s, d_rep_e},
                    d_cls, hipMemcpyDeviceToDevice, read_touch, read_repeat, read_flags, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return ovl_run(c, a);
}

// The same from host arrays, staged through buffers of the context that no pass uses (q_len, q_col, q_csr_a).
int raft_hip_repeat_overlaps_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid, const int32_t *qs,
                                  const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te, int32_t symmetric, int32_t min_anchor,
                                  int64_t n_rep, const int64_t *rep_offset, const int32_t *rep_s, const int32_t *rep_e, uint8_t *cls, int32_t *read_touch,
                                  int32_t *read_repeat, uint8_t *read_flags, raft_hip_ovl_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    OvlCall a{n_reads, read_len, {n_rec, {qid, qs, qe, tid, ts, te}}, symmetric, min_anchor, {n_rep, rep_offset, rep_s, rep_e},
              cls, hipMemcpyDeviceToHost, read_touch, read_repeat, read_flags, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
    PHASE(stage_columns(c, c->q_col, a.rec));
    if (n_rep != -1) PHASE(stage_csr(c, c->q_csr_a, a.rep, n_reads));
    return ovl_run(c, a);
}

} // extern "C"
