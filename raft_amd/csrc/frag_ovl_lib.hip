// frag_ovl_lib.hip -- libraft_hip_frag.so: raft_hip_frag_overlaps_device / _host (include/raft_hip_frag.h), the record stream joined
// with the fragment table.
//
// A library of its own beside libraft_hip.so, as libraft_hip_low.so and libraft_hip_ovl.so are: the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this query needs nothing of the engine but the context it is handed -- the fragment rows and
// the repeat arrays a finished pass left (engine_ctx.hpp), the stream, and buffers of its own registered with the context like every
// other (fo_*).
#include "engine_ctx.hpp"
#include "../../include/raft_hip_frag.h"
#include "frag_ovl.hpp"

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

struct FragCall {
    int32_t n_reads; const int32_t *len; int64_t n_rec; const int32_t *col[6];
    int32_t symmetric;
    int64_t n_frag; const int64_t *frag_off; const int32_t *fb, *fe;          // device arrays, or all NULL with n_frag = -1: the context's pass
    int64_t n_rep; const int64_t *rep_off; const int32_t *rep_s, *rep_e;      // the same; all NULL with n_rep = 0: no annotation
    int32_t *frag_out[4]; hipMemcpyKind frag_kind;                            // touch, span, contained, repeat
    int32_t *read_contained;
    raft_hip_frag_summary *sum; int64_t *error_index; double *kernel_seconds;
};

// three arrays of a CSR table: all of them, or -- where there is nothing for the two row arrays to point at -- the offsets alone
bool csr_given(int64_t count, const void *off, const void *x, const void *y)
{
    if (!off || (x == nullptr) != (y == nullptr)) return false;
    return count == 0 || x != nullptr;
}

// what both forms check before anything is staged: counts, columns, the table and the annotation, the state an own-pass call needs
int check_call(raft_hip_ctx *c, const FragCall &a)
{
    if (!c || a.n_reads < 0 || a.n_rec < 0 || (a.n_reads > 0 && !a.len)) return RAFT_HIP_ERR_PARAM;
    if (a.n_rec > 0)
        for (int k = 0; k < 6; ++k)
            if (!a.col[k]) return RAFT_HIP_ERR_PARAM;
    const bool own_table = a.n_frag == -1, own_rep = a.n_rep == -1;
    const bool no_table = !a.frag_off && !a.fb && !a.fe, no_rep = !a.rep_off && !a.rep_s && !a.rep_e;
    if (a.n_frag < -1 || a.n_rep < -1) return RAFT_HIP_ERR_PARAM;
    if (own_table ? !no_table : !csr_given(a.n_frag, a.frag_off, a.fb, a.fe)) return RAFT_HIP_ERR_PARAM;
    if (own_rep ? !no_rep : !(a.n_rep == 0 && no_rep) && !csr_given(a.n_rep, a.rep_off, a.rep_s, a.rep_e)) return RAFT_HIP_ERR_PARAM;
    if (a.n_rec >= (int64_t(1) << 30) || a.n_frag >= (int64_t(1) << 31) - 1) return RAFT_HIP_ERR_TOO_LARGE;
    if (own_table || own_rep) {                               // the context's own finished pass
        if (!c->finished || c->pending_err) return RAFT_HIP_ERR_STATE;
        if (a.n_reads != c->sum.n_reads) return RAFT_HIP_ERR_PARAM;
        if (own_table && c->sum.n_fragments >= (int64_t(1) << 31) - 1) return RAFT_HIP_ERR_TOO_LARGE;
    }
    return RAFT_HIP_OK;
}

int frag_run(raft_hip_ctx *c, const FragCall &a)
{
    const bool own_table = a.n_frag == -1, own_rep = a.n_rep == -1;
    const long long *off = own_table ? c->frag_off.as<long long>() : reinterpret_cast<const long long *>(a.frag_off);
    const int32_t *fb = own_table ? c->frag_begin.as<int32_t>() : a.fb, *fe = own_table ? c->frag_end.as<int32_t>() : a.fe;
    const long long n_frag = own_table ? c->sum.n_fragments : a.n_frag;
    const long long *rep_off = own_rep ? c->rep_off.as<long long>() : reinterpret_cast<const long long *>(a.rep_off);
    const int32_t *rep_s = own_rep ? c->rep_s.as<int32_t>() : a.rep_s, *rep_e = own_rep ? c->rep_e.as<int32_t>() : a.rep_e;
    const long long n_rep = own_rep ? c->sum.n_repeats : a.n_rep;
    const size_t n = (size_t)std::max(a.n_reads, 1), nf = (size_t)std::max<long long>(n_frag, 1);
    const int scan_nb = std::max(scan_blocks(n_frag), 1);
    HIP_TRY(c, c->fo_digest.ensure(n * sizeof(FragDigest)));
    HIP_TRY(c, c->fo_rep_digest.ensure(n * sizeof(OvlDigest)));
    HIP_TRY(c, c->fo_whole.ensure(n * 4)); HIP_TRY(c, c->fo_read.ensure(n * 4));
    HIP_TRY(c, c->fo_slot.ensure((nf + 1) * sizeof(FragSlot)));
    for (DevBuf &b : c->fo_out) HIP_TRY(c, b.ensure(nf * 4));
    HIP_TRY(c, c->fo_scan.ensure(((size_t)scan_nb * 3 + 3) * 8));
    HIP_TRY(c, c->fo_ctl.ensure((size_t)kFragCtlWords * 8));
    if (a.kernel_seconds && !c->ev_hist0) { HIP_TRY(c, hipEventCreate(&c->ev_hist0)); HIP_TRY(c, hipEventCreate(&c->ev_hist1)); }
    unsigned long long *ctl = c->fo_ctl.as<unsigned long long>();
    int32_t *out[4];
    for (int k = 0; k < 4; ++k) out[k] = c->fo_out[k].as<int32_t>();
    if (a.kernel_seconds) HIP_TRY(c, hipEventRecord(c->ev_hist0, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->fo_slot.p, 0, ((size_t)n_frag + 1) * sizeof(FragSlot), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->fo_whole.p, 0, n * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(ctl, 0xFF, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(ctl + 1, 0, (size_t)(kFragCtlWords - 1) * 8, c->stream));
    const dim3 per_read((unsigned)(((long long)a.n_reads + 1 + 255) / 256));
    if (a.n_reads > 0 || !own_table)
        hipLaunchKernelGGL(frag_digest_kernel, per_read, dim3(256), 0, c->stream, off, fb, fe, a.n_reads, n_frag, c->fo_digest.as<FragDigest>(), ctl);
    if (rep_off && (a.n_reads > 0 || !own_rep))
        hipLaunchKernelGGL(ovl_digest_kernel, per_read, dim3(256), 0, c->stream, rep_off, rep_s, rep_e, a.n_reads, n_rep, c->fo_rep_digest.as<OvlDigest>(),
                           ctl + (kFragBadRepeats - kOvlBadOffsets));
    if (a.n_rec > 0) {
        FragArgs A{a.len, a.col[0], a.col[1], a.col[2], a.col[3], a.col[4], a.col[5], (long long)a.n_rec, a.n_reads, a.symmetric ? 1 : 0,
                   fb, fe, c->fo_digest.as<FragDigest>(), c->fo_slot.as<FragSlot>(), c->fo_whole.as<unsigned>(), ctl};
        uintptr_t bits = 0;
        for (int k = 0; k < 6; ++k) bits |= reinterpret_cast<uintptr_t>(a.col[k]);
        if (bits & 15) hipLaunchKernelGGL(frag_side_kernel<false>, dim3(frag_grid(a.n_rec)), dim3(kFragThreads), 0, c->stream, A);
        else hipLaunchKernelGGL(frag_side_kernel<true>, dim3(frag_grid(a.n_rec)), dim3(kFragThreads), 0, c->stream, A);
    }
    if (n_frag > 0) {                                         // the three difference arrays -> counts (the slot behind the last row only ends ranges)
        const FragLoader ld{c->fo_slot.as<FragSlot>()};
        const FragCounts counts{out[0], out[1], out[2]};
        long long *partials = c->fo_scan.as<long long>();
        hipLaunchKernelGGL((scan_partials_kernel<FragLoader, 3>), dim3(scan_nb), dim3(kScanThreads), 0, c->stream, ld, n_frag, partials, 0x7fffffff, NoBeside());
        hipLaunchKernelGGL((scan_apply_kernel<FragLoader, 3, true, FragCounts>), dim3(scan_nb), dim3(kScanThreads), 0, c->stream, ld, n_frag, partials,
                           partials + (long long)scan_nb * 3, ScanOut<3>{{nullptr, nullptr, nullptr}}, counts);
    }
    if (a.n_reads > 0) {
        FragReadsArgs R{off, fb, fe, a.n_reads, out[0], out[1], out[2], rep_off, rep_s, rep_e, c->fo_rep_digest.as<OvlDigest>(), c->fo_whole.as<unsigned>(),
                        out[3], c->fo_read.as<int32_t>(), ctl};
        hipLaunchKernelGGL(frag_reads_kernel, dim3((unsigned)std::min<long long>(((long long)a.n_reads + 255) / 256, 2048)), dim3(256), 0, c->stream, R);
    }
    HIP_TRY(c, hipGetLastError());
    if (a.kernel_seconds) HIP_TRY(c, hipEventRecord(c->ev_hist1, c->stream));
    unsigned long long h_ctl[kFragCtlWords] = {};
    HIP_TRY(c, hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.kernel_seconds) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_hist0, c->ev_hist1));
        *a.kernel_seconds = ms * 1e-3;
    }
    if (h_ctl[kFragBadTable]) {
        c->last_error = "fragment_overlaps: frag_offset does not begin at 0, ascend and end at n_frag, or a read's rows descend or are not 0 <= begin <= end";
        return RAFT_HIP_ERR_PARAM;
    }
    if (h_ctl[kFragBadRepeats]) {
        c->last_error = "fragment_overlaps: rep_offset does not begin at 0, ascend and end at n_rep";
        return RAFT_HIP_ERR_PARAM;
    }
    if (h_ctl[kFragFirstBad] != ~0ull) {
        if (a.error_index) *a.error_index = (int64_t)h_ctl[kFragFirstBad];
        c->last_error = "fragment_overlaps: a record names a read id outside [0, n_reads)";
        return RAFT_HIP_ERR_READ_ID;
    }
    if (a.error_index) *a.error_index = -1;
    for (int k = 0; k < 4; ++k) PHASE(queue_copy(c, a.frag_out[k], out[k], (size_t)n_frag * 4, a.frag_kind));
    PHASE(queue_copy(c, a.read_contained, c->fo_read.p, (size_t)a.n_reads * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum) {
        const unsigned long long *t = h_ctl + kFragTotals;
        a.sum->n_records = a.n_rec; a.sum->n_fragments = n_frag;
        a.sum->frags_untouched = (int64_t)t[0]; a.sum->frags_spanned = (int64_t)t[1]; a.sum->frags_contained = (int64_t)t[2];
        a.sum->frags_contained_repeat = (int64_t)t[3]; a.sum->reads_whole_spanned = (int64_t)t[4]; a.sum->reads_any_contained = (int64_t)t[5];
        a.sum->reads_all_contained = (int64_t)t[6];
    }
    return RAFT_HIP_OK;
}

FragCall make_call(int32_t n_reads, const int32_t *len, const raft_hip_records *rec, int32_t symmetric, const raft_hip_frag_table *table,
                   const raft_hip_frag_repeats *rep, int32_t *touch, int32_t *span, int32_t *contained, int32_t *repeat, hipMemcpyKind kind,
                   int32_t *read_contained, raft_hip_frag_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    return FragCall{n_reads, len, rec->n_rec, {rec->d_qid, rec->d_qs, rec->d_qe, rec->d_tid, rec->d_ts, rec->d_te}, symmetric,
                    table->n_frag, table->frag_offset, table->frag_begin, table->frag_end, rep->n_rep, rep->rep_offset, rep->rep_s, rep->rep_e,
                    {touch, span, contained, repeat}, kind, read_contained, sum, error_index, kernel_seconds};
}

} // namespace

extern "C" {

int raft_hip_frag_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_frag_overlaps_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, const raft_hip_records *records, int32_t symmetric,
                                  const raft_hip_frag_table *table, const raft_hip_frag_repeats *repeats, int32_t *d_frag_touch, int32_t *d_frag_span,
                                  int32_t *d_frag_contained, int32_t *d_frag_repeat, int32_t *read_contained, raft_hip_frag_summary *sum,
                                  int64_t *error_index, double *kernel_seconds)
{
    if (!records || !table || !repeats) return RAFT_HIP_ERR_PARAM;
    const FragCall a = make_call(n_reads, d_read_len, records, symmetric, table, repeats, d_frag_touch, d_frag_span, d_frag_contained, d_frag_repeat,
                                 hipMemcpyDeviceToDevice, read_contained, sum, error_index, kernel_seconds);
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return frag_run(c, a);
}

// The same from host arrays, staged through buffers of the context that no pass uses (fo_len, fo_col, fo_tab_*, fo_rep_*).
int raft_hip_frag_overlaps_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, const raft_hip_records *records, int32_t symmetric,
                                const raft_hip_frag_table *table, const raft_hip_frag_repeats *repeats, int32_t *frag_touch, int32_t *frag_span,
                                int32_t *frag_contained, int32_t *frag_repeat, int32_t *read_contained, raft_hip_frag_summary *sum,
                                int64_t *error_index, double *kernel_seconds)
{
    if (!records || !table || !repeats) return RAFT_HIP_ERR_PARAM;
    FragCall a = make_call(n_reads, read_len, records, symmetric, table, repeats, frag_touch, frag_span, frag_contained, frag_repeat,
                           hipMemcpyDeviceToHost, read_contained, sum, error_index, kernel_seconds);
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    auto stage = [&](DevBuf &buf, const void *src, size_t count, size_t elem, const void **dev) -> int {
        HIP_TRY(c, buf.ensure(std::max<size_t>(count, 1) * elem));
        if (count > 0 && src) HIP_TRY(c, hipMemcpyAsync(buf.p, src, count * elem, hipMemcpyHostToDevice, c->stream));
        *dev = buf.p;
        return RAFT_HIP_OK;
    };
    PHASE(stage(c->fo_len, read_len, (size_t)n_reads, 4, reinterpret_cast<const void **>(&a.len)));
    for (int k = 0; k < 6; ++k) PHASE(stage(c->fo_col[k], a.col[k], (size_t)a.n_rec, 4, reinterpret_cast<const void **>(&a.col[k])));
    if (a.n_frag != -1) {
        PHASE(stage(c->fo_tab_off, a.frag_off, (size_t)n_reads + 1, 8, reinterpret_cast<const void **>(&a.frag_off)));
        PHASE(stage(c->fo_tab_b, a.fb, (size_t)a.n_frag, 4, reinterpret_cast<const void **>(&a.fb)));
        PHASE(stage(c->fo_tab_e, a.fe, (size_t)a.n_frag, 4, reinterpret_cast<const void **>(&a.fe)));
    }
    if (a.n_rep != -1 && a.rep_off) {
        PHASE(stage(c->fo_rep_off, a.rep_off, (size_t)n_reads + 1, 8, reinterpret_cast<const void **>(&a.rep_off)));
        PHASE(stage(c->fo_rep_s, a.rep_s, (size_t)a.n_rep, 4, reinterpret_cast<const void **>(&a.rep_s)));
        PHASE(stage(c->fo_rep_e, a.rep_e, (size_t)a.n_rep, 4, reinterpret_cast<const void **>(&a.rep_e)));
    }
    return frag_run(c, a);
}

} // extern "C"
