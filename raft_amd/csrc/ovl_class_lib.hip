// ovl_class_lib.hip -- libraft_hip_ovl.so: raft_hip_repeat_overlaps_device / _host (include/raft_hip_ovl.h), the record stream
// classified against the repeat annotation.
//
// A library of its own beside libraft_hip.so, as libraft_hip_low.so is: the set of entry points of include/raft_hip.h is closed
// (ABI 11), and this query needs nothing of the engine but the context it is handed -- the repeat arrays a finished pass left
// (engine_ctx.hpp), the stream, and buffers of its own registered with the context like every other (oc_*).
#include "engine_ctx.hpp"
#include "../../include/raft_hip_ovl.h"
#include "ovl_class.hpp"

#include <algorithm>

namespace {

#define PHASE(expr)                                              \
    do {                                                         \
        const int rc_ = (expr);                                  \
        if (rc_ != RAFT_HIP_OK) return rc_;                      \
    } while (0)

// a destination the caller left NULL, or nothing to copy, is skipped
int queue_copy(raft_hip_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    if (dst && bytes) HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    return RAFT_HIP_OK;
}

struct OvlCall {
    int32_t n_reads; const int32_t *len; int64_t n_rec; const int32_t *col[6];
    int32_t symmetric, min_anchor;
    int64_t n_rep; const int64_t *rep_off; const int32_t *rep_s, *rep_e;      // device arrays, or all NULL with n_rep = -1: the context's pass
    uint8_t *cls; hipMemcpyKind cls_kind;
    int32_t *read_touch, *read_repeat; uint8_t *read_flags;
    raft_hip_ovl_summary *sum; int64_t *error_index; double *kernel_seconds;
};

// what both forms check before anything is staged: counts, columns, the three repeat arrays, the state an own-pass call needs
int check_call(raft_hip_ctx *c, const OvlCall &a)
{
    if (!c || a.n_reads < 0 || a.n_rec < 0 || a.min_anchor < 1 || (a.n_reads > 0 && !a.len)) return RAFT_HIP_ERR_PARAM;
    if (a.n_rec > 0 && (!a.col[0] || !a.col[1] || !a.col[2] || !a.col[3])) return RAFT_HIP_ERR_PARAM;
    if ((a.col[4] == nullptr) != (a.col[5] == nullptr)) return RAFT_HIP_ERR_PARAM;
    if (a.n_rec > 0 && !a.symmetric && !a.col[4]) return RAFT_HIP_ERR_PARAM;
    const int given = (a.rep_off ? 1 : 0) + (a.rep_s ? 1 : 0) + (a.rep_e ? 1 : 0);
    if (given == 0 && a.n_rep == -1) {                        // the context's own finished pass
        if (!c->finished || c->pending_err) return RAFT_HIP_ERR_STATE;
        if (a.n_reads != c->sum.n_reads) return RAFT_HIP_ERR_PARAM;
        return RAFT_HIP_OK;
    }
    if (a.n_rep < 0 || !a.rep_off) return RAFT_HIP_ERR_PARAM;
    if (a.n_rep > 0 ? given != 3 : (given != 1 && given != 3)) return RAFT_HIP_ERR_PARAM;      // (no run: rep_s / rep_e have nothing to point at)
    return RAFT_HIP_OK;
}

int ovl_run(raft_hip_ctx *c, const OvlCall &a)
{
    const bool own = a.n_rep == -1;
    const long long *rep_off = own ? c->rep_off.as<long long>() : reinterpret_cast<const long long *>(a.rep_off);
    const int32_t *rep_s = own ? c->rep_s.as<int32_t>() : a.rep_s, *rep_e = own ? c->rep_e.as<int32_t>() : a.rep_e;
    const long long n_rep = own ? c->sum.n_repeats : a.n_rep;
    const size_t n = (size_t)std::max(a.n_reads, 1);
    HIP_TRY(c, c->oc_digest.ensure(n * sizeof(OvlDigest)));
    HIP_TRY(c, c->oc_touch.ensure(n * 4)); HIP_TRY(c, c->oc_repeat.ensure(n * 4)); HIP_TRY(c, c->oc_flagw.ensure(n * 4));
    HIP_TRY(c, c->oc_tally.ensure(n * 8));
    HIP_TRY(c, c->oc_flags.ensure(n));
    HIP_TRY(c, c->oc_ctl.ensure((size_t)kOvlCtlWords * 8));
    if (a.cls) HIP_TRY(c, c->oc_cls.ensure((size_t)std::max<int64_t>(a.n_rec, 1) + 4));
    if (a.kernel_seconds && !c->ev_hist0) { HIP_TRY(c, hipEventCreate(&c->ev_hist0)); HIP_TRY(c, hipEventCreate(&c->ev_hist1)); }
    unsigned long long *ctl = c->oc_ctl.as<unsigned long long>();
    HIP_TRY(c, hipMemsetAsync(c->oc_tally.p, 0, n * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->oc_flagw.p, 0, n * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(ctl, 0xFF, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(ctl + 1, 0, (size_t)(kOvlCtlWords - 1) * 8, c->stream));
    if (a.kernel_seconds) HIP_TRY(c, hipEventRecord(c->ev_hist0, c->stream));
    if (a.n_reads > 0 || !own)
        hipLaunchKernelGGL(ovl_digest_kernel, dim3((unsigned)(((long long)a.n_reads + 1 + 255) / 256)), dim3(256), 0, c->stream, rep_off, rep_s, rep_e,
                           a.n_reads, n_rep, c->oc_digest.as<OvlDigest>(), ctl);
    if (a.n_rec > 0) {
        OvlArgs A{a.len, a.col[0], a.col[1], a.col[2], a.col[3], a.col[4], a.col[5], (long long)a.n_rec, a.n_reads, a.symmetric ? 1 : 0, a.min_anchor,
                  rep_off, rep_s, rep_e, c->oc_digest.as<OvlDigest>(), a.cls ? c->oc_cls.as<uint8_t>() : nullptr,
                  c->oc_tally.as<unsigned long long>(), c->oc_flagw.as<unsigned>(), ctl};
        uintptr_t bits = 0;
        for (int k = 0; k < 6; ++k) bits |= reinterpret_cast<uintptr_t>(a.col[k]);
        if (bits & 15) hipLaunchKernelGGL(ovl_class_kernel<false>, dim3(ovl_grid(a.n_rec)), dim3(kOvlThreads), 0, c->stream, A);
        else hipLaunchKernelGGL(ovl_class_kernel<true>, dim3(ovl_grid(a.n_rec)), dim3(kOvlThreads), 0, c->stream, A);
    }
    if (a.n_reads > 0)
        hipLaunchKernelGGL(ovl_reads_kernel, dim3((unsigned)std::min<long long>(((long long)a.n_reads + 255) / 256, 1024)), dim3(256), 0, c->stream,
                           c->oc_flagw.as<unsigned>(), c->oc_tally.as<unsigned long long>(), a.n_reads, c->oc_flags.as<uint8_t>(),
                           c->oc_touch.as<int32_t>(), c->oc_repeat.as<int32_t>(), ctl);
    HIP_TRY(c, hipGetLastError());
    if (a.kernel_seconds) HIP_TRY(c, hipEventRecord(c->ev_hist1, c->stream));
    unsigned long long h_ctl[kOvlCtlWords] = {};
    HIP_TRY(c, hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.kernel_seconds) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_hist0, c->ev_hist1));
        *a.kernel_seconds = ms * 1e-3;
    }
    if (h_ctl[kOvlBadOffsets]) {
        c->last_error = "repeat_overlaps: rep_offset does not begin at 0, ascend and end at n_rep";
        return RAFT_HIP_ERR_PARAM;
    }
    if (h_ctl[kOvlFirstBad] != ~0ull) {
        if (a.error_index) *a.error_index = (int64_t)h_ctl[kOvlFirstBad];
        c->last_error = "repeat_overlaps: a record names a read id outside [0, n_reads)";
        return RAFT_HIP_ERR_READ_ID;
    }
    if (a.error_index) *a.error_index = -1;
    if (a.n_rec > 0) PHASE(queue_copy(c, a.cls, c->oc_cls.p, (size_t)a.n_rec, a.cls_kind));
    PHASE(queue_copy(c, a.read_touch, c->oc_touch.p, (size_t)a.n_reads * 4, hipMemcpyDeviceToHost));
    PHASE(queue_copy(c, a.read_repeat, c->oc_repeat.p, (size_t)a.n_reads * 4, hipMemcpyDeviceToHost));
    PHASE(queue_copy(c, a.read_flags, c->oc_flags.p, (size_t)a.n_reads, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum) {
        const unsigned long long *t = h_ctl + kOvlRecTotals;
        a.sum->n_records = a.n_rec;
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
    const OvlCall a{n_reads, d_read_len, n_rec, {d_qid, d_qs, d_qe, d_tid, d_ts, d_te}, symmetric, min_anchor, n_rep, d_rep_offset, d_rep_s, d_rep_e,
                    d_cls, hipMemcpyDeviceToDevice, read_touch, read_repeat, read_flags, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return ovl_run(c, a);
}

// The same from host arrays, staged through buffers of the context that no pass uses (oc_len, oc_col, oc_rep_*).
int raft_hip_repeat_overlaps_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid, const int32_t *qs,
                                  const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te, int32_t symmetric, int32_t min_anchor,
                                  int64_t n_rep, const int64_t *rep_offset, const int32_t *rep_s, const int32_t *rep_e, uint8_t *cls, int32_t *read_touch,
                                  int32_t *read_repeat, uint8_t *read_flags, raft_hip_ovl_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    OvlCall a{n_reads, read_len, n_rec, {qid, qs, qe, tid, ts, te}, symmetric, min_anchor, n_rep, rep_offset, rep_s, rep_e,
              cls, hipMemcpyDeviceToHost, read_touch, read_repeat, read_flags, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    auto stage = [&](DevBuf &buf, const void *src, size_t count, size_t elem, const void **dev) -> int {
        HIP_TRY(c, buf.ensure(std::max<size_t>(count, 1) * elem));
        if (count > 0) HIP_TRY(c, hipMemcpyAsync(buf.p, src, count * elem, hipMemcpyHostToDevice, c->stream));
        *dev = buf.p;
        return RAFT_HIP_OK;
    };
    PHASE(stage(c->oc_len, read_len, (size_t)n_reads, 4, reinterpret_cast<const void **>(&a.len)));
    for (int k = 0; k < 6; ++k)
        if (a.col[k] || k < 4) PHASE(stage(c->oc_col[k], a.col[k], (size_t)n_rec, 4, reinterpret_cast<const void **>(&a.col[k])));
    if (n_rep != -1) {
        PHASE(stage(c->oc_rep_off, rep_offset, (size_t)n_reads + 1, 8, reinterpret_cast<const void **>(&a.rep_off)));
        PHASE(stage(c->oc_rep_s, rep_s, (size_t)n_rep, 4, reinterpret_cast<const void **>(&a.rep_s)));
        PHASE(stage(c->oc_rep_e, rep_e, (size_t)n_rep, 4, reinterpret_cast<const void **>(&a.rep_e)));
    }
    return ovl_run(c, a);
}

} // extern "C"
