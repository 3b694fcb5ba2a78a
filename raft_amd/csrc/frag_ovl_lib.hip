// frag_ovl_lib.hip -- libraft_hip_frag.so: raft_hip_frag_overlaps_device / _host (include/raft_hip_frag.h), the record stream joined
// with the fragment table.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this query needs nothing of the engine but the context it is handed -- the fragment rows
// and the repeat arrays a finished pass left (engine_ctx.hpp), the stream, and buffers registered with the context like every other
// (fo_*, and the queries' shared staging q_*).
#include "query_host.hpp"
#include "../../include/raft_hip_frag.h"
#include "frag_ovl.hpp"

#include <algorithm>

namespace {

struct FragCall {
    int32_t n_reads; const int32_t *len; RecordCols rec;
    int32_t symmetric;
    CsrArg table;                                                             // device arrays, or all NULL with count -1: the context's pass
    CsrArg rep;                                                               // the same; all NULL with count 0: no annotation
    int32_t *frag_out[4]; hipMemcpyKind frag_kind;                            // touch, span, contained, repeat
    int32_t *read_contained;
    raft_hip_frag_summary *sum; int64_t *error_index; double *kernel_seconds;
};

// what both forms check before anything is staged: counts, columns, the table and the annotation, the state an own-pass call needs
int check_call(raft_hip_ctx *c, const FragCall &a)
{
    const char *who = "fragment_overlaps";
    if (!c || a.n_reads < 0 || a.rec.n_rec < 0 || (a.n_reads > 0 && !a.len)) return refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);
    if (!record_cols_ok(a.rec, a.symmetric != 0, TargetCols::always)) return refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);
    const CsrKind table = csr_arg_kind(a.table), rep = csr_arg_kind(a.rep);
    if (table == CsrKind::bad || table == CsrKind::none || rep == CsrKind::bad) return refuse(c, RAFT_HIP_ERR_PARAM, who, kBadArgs);    // (the annotation may be left out)
    const bool own_table = table == CsrKind::own, own_rep = rep == CsrKind::own;
    if (a.rec.n_rec >= (int64_t(1) << 30) || a.table.count >= (int64_t(1) << 31) - 1) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, who, "too many records or rows");
    if (own_table || own_rep) {                               // the context's own finished pass
        if (!c->finished || c->pending_err) return refuse(c, RAFT_HIP_ERR_STATE, who, kNoPass);
        if (a.n_reads != c->sum.n_reads) return refuse(c, RAFT_HIP_ERR_PARAM, who, kOtherReads);
        if (own_table && c->sum.n_fragments >= (int64_t(1) << 31) - 1) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, who, "too many records or rows");
    }
    return RAFT_HIP_OK;
}

int frag_run(raft_hip_ctx *c, const FragCall &a)
{
    const bool own_table = a.table.count == -1, own_rep = a.rep.count == -1;
    const CsrDev table = resolve_csr(a.table, c->frag_off, c->frag_begin, c->frag_end, c->sum.n_fragments);
    const CsrDev rep = resolve_csr(a.rep, c->rep_off, c->rep_s, c->rep_e, c->sum.n_repeats);
    const long long n_frag = table.count;
    const int64_t n_rec = a.rec.n_rec;
    const int32_t *const *col = a.rec.col;
    const size_t n = (size_t)std::max(a.n_reads, 1), nf = (size_t)std::max<long long>(n_frag, 1);
    const int scan_nb = std::max(scan_blocks(n_frag), 1);
    HIP_TRY(c, c->fo_digest.ensure(n * sizeof(FragDigest)));
    HIP_TRY(c, c->fo_rep_digest.ensure(n * sizeof(OvlDigest)));
    HIP_TRY(c, c->fo_whole.ensure(n * 4)); HIP_TRY(c, c->fo_read.ensure(n * 4));
    HIP_TRY(c, c->fo_slot.ensure((nf + 1) * sizeof(FragSlot)));
    for (DevBuf &b : c->fo_out) HIP_TRY(c, b.ensure(nf * 4));
    HIP_TRY(c, c->fo_scan.ensure(((size_t)scan_nb * 3 + 3) * 8));
    HIP_TRY(c, c->fo_ctl.ensure((size_t)kFragCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    unsigned long long *ctl = c->fo_ctl.as<unsigned long long>();
    int32_t *out[4];
    for (int k = 0; k < 4; ++k) out[k] = c->fo_out[k].as<int32_t>();
    PHASE(timer.start());
    HIP_TRY(c, hipMemsetAsync(c->fo_slot.p, 0, ((size_t)n_frag + 1) * sizeof(FragSlot), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->fo_whole.p, 0, n * 4, c->stream));
    PHASE(clear_ctl(c, ctl, kFragCtlWords));
    const dim3 per_read((unsigned)(((long long)a.n_reads + 1 + 255) / 256));
    if (a.n_reads > 0 || !own_table)
        hipLaunchKernelGGL(frag_digest_kernel, per_read, dim3(256), 0, c->stream, table.off, table.x, table.y, a.n_reads, n_frag, c->fo_digest.as<FragDigest>(), ctl);
    if (rep.off && (a.n_reads > 0 || !own_rep))
        hipLaunchKernelGGL(ovl_digest_kernel, per_read, dim3(256), 0, c->stream, rep.off, rep.x, rep.y, a.n_reads, rep.count, c->fo_rep_digest.as<OvlDigest>(),
                           ctl + (kFragBadRepeats - kOvlBadOffsets));
    if (n_rec > 0) {
        FragArgs A{a.len, col[0], col[1], col[2], col[3], col[4], col[5], (long long)n_rec, a.n_reads, a.symmetric ? 1 : 0,
                   table.x, table.y, c->fo_digest.as<FragDigest>(), c->fo_slot.as<FragSlot>(), c->fo_whole.as<unsigned>(), ctl};
        if (aligned16(a.rec)) hipLaunchKernelGGL(frag_side_kernel<true>, dim3(stream_grid(n_rec)), dim3(kStreamThreads), 0, c->stream, A);
        else hipLaunchKernelGGL(frag_side_kernel<false>, dim3(stream_grid(n_rec)), dim3(kStreamThreads), 0, c->stream, A);
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
        FragReadsArgs R{table.off, table.x, table.y, a.n_reads, out[0], out[1], out[2], rep.off, rep.x, rep.y, c->fo_rep_digest.as<OvlDigest>(), c->fo_whole.as<unsigned>(),
                        out[3], c->fo_read.as<int32_t>(), ctl};
        hipLaunchKernelGGL(frag_reads_kernel, dim3((unsigned)std::min<long long>(((long long)a.n_reads + 255) / 256, 2048)), dim3(256), 0, c->stream, R);
    }
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kFragCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kFragCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(a.kernel_seconds));
    if (h_ctl[kFragBadTable]) {
        c->last_error = "fragment_overlaps: frag_offset does not begin at 0, ascend and end at n_frag, or a read's rows descend or are not 0 <= begin <= end";
        return RAFT_HIP_ERR_PARAM;
    }
    if (h_ctl[kFragBadRepeats]) {
        c->last_error = "fragment_overlaps: rep_offset does not begin at 0, ascend and end at n_rep";
        return RAFT_HIP_ERR_PARAM;
    }
    PHASE(first_bad_record(c, h_ctl[kFragFirstBad], a.error_index, "fragment_overlaps: a record names a read id outside [0, n_reads)"));
    for (int k = 0; k < 4; ++k) PHASE(queue_copies(c, {{a.frag_out[k], out[k], (size_t)n_frag * 4, a.frag_kind}}));
    PHASE(queue_copies(c, {{a.read_contained, c->fo_read.p, (size_t)a.n_reads * 4}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum) {
        const unsigned long long *t = h_ctl + kFragTotals;
        a.sum->n_records = n_rec; a.sum->n_fragments = n_frag;
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
    return FragCall{n_reads, len, {rec->n_rec, {rec->d_qid, rec->d_qs, rec->d_qe, rec->d_tid, rec->d_ts, rec->d_te}}, symmetric,
                    {table->n_frag, table->frag_offset, table->frag_begin, table->frag_end}, {rep->n_rep, rep->rep_offset, rep->rep_s, rep->rep_e},
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

// The same from host arrays, staged through buffers of the context that no pass uses (q_len, q_col, q_csr_a, q_csr_b).
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
    PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
    PHASE(stage_columns(c, c->q_col, a.rec));
    if (csr_arg_kind(a.table) == CsrKind::given) PHASE(stage_csr(c, c->q_csr_a, a.table, n_reads));
    if (csr_arg_kind(a.rep) == CsrKind::given) PHASE(stage_csr(c, c->q_csr_b, a.rep, n_reads));
    return frag_run(c, a);
}

} // extern "C"
