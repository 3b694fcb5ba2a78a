// components_lib.hip -- libraft_hip_cc.so: raft_hip_components_device / _host (include/raft_hip_cc.h), the connected components of the
// graph whose edges are the records of a stream with a kind in the mask.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this call needs nothing of the engine but the context it is handed -- the stream, and
// buffers registered with the context like every other (cc_*, and the queries' shared staging q_len, q_col).  It reads no finished
// pass and leaves the context's state as it is.
#include "query_host.hpp"
#include "../../include/raft_hip_cc.h"
#include "device_scan.hpp"
#include "components.hpp"

namespace {

struct CcCall {
    int32_t n_reads;
    const int32_t *len;
    RecordCols rec;
    const uint8_t *strand;
    int32_t max_overhang, min_ratio, kind_mask, symmetric;
    int32_t *component, *degree, *comp_first, *comp_reads; int64_t *comp_bases, *comp_sides;
    raft_hip_cc_summary *sum; int64_t *error_index; double *kernel_seconds; int64_t *launches;
};

constexpr const char *kWho = "components";
static_assert(RAFT_HIP_CC_KINDS_ALL == kCcKindBits && RAFT_HIP_CC_KINDS_PROPER == (kCcKindBits & ~(1 << kEndInternal)), "the masks of the header");

// what both forms check before anything is staged
int check_call(raft_hip_ctx *c, const CcCall &a)
{
    PHASE(check_ends_rule_call(c, kWho, a.max_overhang, a.min_ratio, a.n_reads, a.len, a.rec, a.strand));
    if (a.kind_mask == 0 || (a.kind_mask & ~kCcKindBits) != 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "kind_mask is 0 or holds a bit other than 1 .. 5");
    return RAFT_HIP_OK;
}

// the four-record loads: the six columns on 16-byte lines, strand on a 4-byte one
bool vector_path(const CcCall &a)
{
    return aligned16(a.rec) && (reinterpret_cast<uintptr_t>(a.strand) & 3) == 0;
}

// a: device arrays but for the outputs
int cc_run(raft_hip_ctx *c, const CcCall &a)
{
    const int64_t n_rec = a.rec.n_rec;
    const size_t n = (size_t)std::max(a.n_reads, 1);
    const int nb = std::max(scan_blocks((long long)a.n_reads), 1);
    HIP_TRY(c, c->cc_parent.ensure(n * 4));
    HIP_TRY(c, c->cc_root.ensure(n * 4));
    HIP_TRY(c, c->cc_degree.ensure(n * 4));
    HIP_TRY(c, c->cc_acc.ensure(n * (8 + 8 + 4)));                        // bases, sides, then reads
    HIP_TRY(c, c->cc_scan.ensure(((n + 1) + (size_t)nb + 1) * 8));       // the roots' prefix, the scan's partial sums and total
    HIP_TRY(c, c->cc_comp.ensure(n * 4));
    HIP_TRY(c, c->cc_rows[0].ensure(n * 4));
    HIP_TRY(c, c->cc_rows[1].ensure(n * 4));
    HIP_TRY(c, c->cc_rows[2].ensure(n * 8));
    HIP_TRY(c, c->cc_rows[3].ensure(n * 8));
    HIP_TRY(c, c->cc_ctl.ensure((size_t)kCcCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    if (a.launches) *a.launches = 0;
    unsigned long long *ctl = c->cc_ctl.as<unsigned long long>();
    int32_t *parent = c->cc_parent.as<int32_t>(), *root = c->cc_root.as<int32_t>();
    unsigned *degree = c->cc_degree.as<unsigned>();
    unsigned long long *acc64 = c->cc_acc.as<unsigned long long>();
    const CcAcc acc{reinterpret_cast<unsigned *>(acc64 + 2 * n), acc64, acc64 + n};
    long long *root_id = c->cc_scan.as<long long>(), *partials = root_id + (n + 1);
    const CcOut out{c->cc_comp.as<int32_t>(), c->cc_rows[0].as<int32_t>(), c->cc_rows[1].as<int32_t>(), c->cc_rows[2].as<long long>(),
                    c->cc_rows[3].as<long long>()};
    int64_t launches = 0;
    PHASE(clear_ctl(c, ctl, kCcCtlWords));
    PHASE(timer.start());
    if (a.n_reads > 0) {
        const dim3 grid(cc_grid(a.n_reads)), block(kCcThreads);
        hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, c->stream, a.n_reads, parent, degree, acc);
        launches += 1;
    }
    if (n_rec > 0) {
        const int32_t *const *col = a.rec.col;
        const CcLinkArgs A{a.len, col[0], col[1], col[2], col[3], col[4], col[5], a.strand, (long long)n_rec, a.n_reads, a.max_overhang,
                           a.min_ratio, a.kind_mask, a.symmetric ? 1 : 0, parent, degree, ctl};
        const dim3 grid(stream_grid(n_rec)), block(kStreamThreads);
        if (vector_path(a)) hipLaunchKernelGGL((cc_link_kernel<true, kCcHalve>), grid, block, 0, c->stream, A);
        else hipLaunchKernelGGL((cc_link_kernel<false, kCcHalve>), grid, block, 0, c->stream, A);
        launches += 1;
    }
    if (a.n_reads > 0) {
        const dim3 grid(cc_grid(a.n_reads)), block(kCcThreads);
        hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, c->stream, parent, a.n_reads, root);
        hipLaunchKernelGGL(cc_sum_kernel, dim3(stream_grid(a.n_reads)), dim3(kStreamThreads), 0, c->stream, root, a.len, degree, a.n_reads, acc);
        exclusive_scan<CcRootLoader, 1>(c->stream, CcRootLoader{root}, (long long)a.n_reads, partials, ScanOut<1>{{root_id}});
        hipLaunchKernelGGL(cc_emit_kernel, grid, block, 0, c->stream, root, a.n_reads, root_id, acc, out, ctl);
        launches += 5;
    }
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kCcCtlWords] = {};
    long long n_comp = 0;
    PHASE(read_ctl(c, ctl, h_ctl, kCcCtlWords));
    if (a.n_reads > 0) PHASE(queue_copies(c, {{&n_comp, root_id + a.n_reads, 8}}));      // C: the scan's last element
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // (the one wait: the first bad record, the totals and C)
    PHASE(timer.seconds(a.kernel_seconds));
    if (a.launches) *a.launches = launches;
    PHASE(first_bad_record(c, h_ctl[0], a.error_index, "components: a record names a read id outside [0, n_reads)"));
    const unsigned long long *t = h_ctl + kCcCtlTotals;
    if (n_comp < 0 || n_comp > a.n_reads || (unsigned long long)n_comp != t[kCcComponents]) {
        c->last_error = "components: the roots' prefix and the emitted rows disagree";
        return RAFT_HIP_ERR_DEVICE;
    }
    const size_t n_reads = (size_t)a.n_reads, C = (size_t)n_comp;
    PHASE(queue_copies(c, {{a.component, out.component, n_reads * 4}, {a.degree, degree, n_reads * 4}, {a.comp_first, out.first, C * 4},
                           {a.comp_reads, out.reads, C * 4}, {a.comp_bases, out.bases, C * 8}, {a.comp_sides, out.sides, C * 8}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum)
        *a.sum = raft_hip_cc_summary{(int64_t)a.n_reads, n_rec, (int64_t)h_ctl[kCcCtlEdges], (int64_t)n_comp, (int64_t)t[kCcSingletons],
                                     (int64_t)t[kCcLargestReads], (int64_t)t[kCcLargestBases], (int64_t)t[kCcTotalBases],
                                     a.n_reads > 0 ? (int64_t)(t[kCcLargestReads] * 1000ull / (unsigned long long)a.n_reads) : 0};
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_cc_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_components_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                               const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                               const uint8_t *d_strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t kind_mask, int32_t symmetric,
                               int32_t *component, int32_t *degree, int32_t *comp_first, int32_t *comp_reads, int64_t *comp_bases,
                               int64_t *comp_sides, raft_hip_cc_summary *sum, int64_t *error_index, double *kernel_seconds, int64_t *launches)
{
    const CcCall a{n_reads, d_read_len, {n_rec, {d_qid, d_qs, d_qe, d_tid, d_ts, d_te}}, d_strand, max_overhang, min_ratio_permille, kind_mask,
                   symmetric, component, degree, comp_first, comp_reads, comp_bases, comp_sides, sum, error_index, kernel_seconds, launches};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return cc_run(c, a);
}

// The same from host arrays: the lengths and the six columns staged through q_len and q_col, which no pass uses, the strand bytes
// through cc_strand.
int raft_hip_components_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                             const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                             const uint8_t *strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t kind_mask, int32_t symmetric,
                             int32_t *component, int32_t *degree, int32_t *comp_first, int32_t *comp_reads, int64_t *comp_bases,
                             int64_t *comp_sides, raft_hip_cc_summary *sum, int64_t *error_index, double *kernel_seconds, int64_t *launches)
{
    CcCall a{n_reads, read_len, {n_rec, {qid, qs, qe, tid, ts, te}}, strand, max_overhang, min_ratio_permille, kind_mask, symmetric,
             component, degree, comp_first, comp_reads, comp_bases, comp_sides, sum, error_index, kernel_seconds, launches};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
    if (n_rec > 0) {
        PHASE(stage_columns(c, c->q_col, a.rec));
        PHASE(stage_host(c, c->cc_strand, strand, (size_t)n_rec, &a.strand));
    }
    return cc_run(c, a);
}

} // extern "C"
