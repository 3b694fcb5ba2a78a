// unitig_lib.hip -- libraft_hip_utg.so: raft_hip_unitigs_device / _host (include/raft_hip_utg.h), the unitigs of the best overlap
// graph.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this call needs nothing of the engine but the context it is handed -- the stream, and
// buffers registered with the context like every other (ut_*, and the queries' shared staging q_len, q_col).  It reads no finished
// pass and leaves the context's state as it is.
#include "query_host.hpp"
#include "../../include/raft_hip_utg.h"
#include "device_scan.hpp"
#include "unitig.hpp"

namespace {

struct UtgCall {
    int32_t n_reads;
    const int32_t *len, *partner, *span;
    const uint8_t *flags;
    int32_t *unitig, *index; int64_t *offset; uint8_t *orient; int32_t *order;
    int64_t *utg_off; int32_t *utg_reads; int64_t *utg_length; uint8_t *utg_circular;
    raft_hip_utg_summary *sum; int64_t *error_index; double *kernel_seconds; int64_t *launches;
};

constexpr const char *kWho = "unitigs";

// what both forms check before anything is staged
int check_call(raft_hip_ctx *c, const UtgCall &a)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (a.n_reads < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "n_reads is negative");
    if (a.n_reads > kUtgMaxReads) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, "more than 2^30 - 1 reads (half-edge ids are int32)");
    if (a.n_reads > 0 && !a.len) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "read_len is missing");
    if (a.n_reads > 0 && (!a.partner || !a.span || !a.flags)) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "a missing array (partner, span, flags)");
    return RAFT_HIP_OK;
}

// one ranking: the init kernel, then the rounds from one half of ut_state into the other -- *final_half is the half the last round
// wrote; with `count` the last round counts the half-edges still under way
void rank(raft_hip_ctx *c, const UtgCall &a, const uint8_t *cut, int rounds, bool count, UtgState **final_half, int64_t *launches)
{
    const long long n_half = 2 * (long long)a.n_reads;
    UtgState *const half[2] = {c->ut_state.as<UtgState>(), c->ut_state.as<UtgState>() + n_half};
    *final_half = utg_rank(c->stream, a.n_reads, a.len, a.partner, a.span, a.flags, cut, half, c->ut_ctl.as<unsigned long long>(), rounds, count, launches);
}

// a: device arrays but for the outputs
int utg_run(raft_hip_ctx *c, const UtgCall &a)
{
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    if (a.launches) *a.launches = 0;
    if (a.n_reads == 0) {
        if (a.utg_off) a.utg_off[0] = 0;
        if (a.sum) *a.sum = raft_hip_utg_summary{};
        if (a.error_index) *a.error_index = -1;
        return RAFT_HIP_OK;
    }
    const size_t n = (size_t)a.n_reads;
    const int nb = std::max(scan_blocks((long long)n), 1);
    HIP_TRY(c, c->ut_state.ensure(n * 4 * sizeof(UtgState)));             // two half-edges per read, two halves
    HIP_TRY(c, c->ut_cut.ensure(n));
    HIP_TRY(c, c->ut_read.ensure(n * sizeof(UtgPlace)));
    HIP_TRY(c, c->ut_offset.ensure(n * 8));
    HIP_TRY(c, c->ut_ulen.ensure(n * 8));
    HIP_TRY(c, c->ut_orient.ensure(n));
    HIP_TRY(c, c->ut_scan.ensure(((n + 1) * 2 + (size_t)nb * 2 + 2) * 8));   // two prefix arrays, the scan's partial sums and totals
    HIP_TRY(c, c->ut_unitig.ensure(n * 2 * 4));                           // unitig, then index
    HIP_TRY(c, c->ut_order.ensure(n * 4));
    HIP_TRY(c, c->ut_utg[0].ensure((n + 1) * 8));
    HIP_TRY(c, c->ut_utg[1].ensure(n * 4));
    HIP_TRY(c, c->ut_utg[2].ensure(n * 8));
    HIP_TRY(c, c->ut_utg[3].ensure(n));
    HIP_TRY(c, c->ut_ctl.ensure((size_t)kUtgCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    unsigned long long *ctl = c->ut_ctl.as<unsigned long long>();
    const int rounds = utg_rounds(a.n_reads);
    int64_t launches = 0;
    double seconds = 0.0, part = 0.0;
    UtgState *state = nullptr;
    // the ranking; the host then reads the first bad read and the number of half-edges on cycles
    PHASE(clear_ctl(c, ctl, kUtgCtlWords));
    PHASE(timer.start());
    rank(c, a, nullptr, rounds, true, &state, &launches);
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kUtgCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kUtgCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(&part));
    seconds += part;
    if (a.launches) *a.launches = launches;
    if (a.kernel_seconds) *a.kernel_seconds = seconds;
    PHASE(first_bad_record(c, h_ctl[0], a.error_index, "unitigs: the table is inconsistent at an end with the MUTUAL bit (error_index: the read)"));
    // cycles: each is cut open at its smallest read and everything is ranked once more
    const uint8_t *cut = nullptr;
    PHASE(timer.start());
    if (h_ctl[kUtgCtlCycle] != 0) {
        hipLaunchKernelGGL(utg_mark_kernel, dim3(utg_grid(a.n_reads)), dim3(kUtgThreads), 0, c->stream, state, a.n_reads, c->ut_cut.as<uint8_t>());
        launches += 1;
        cut = c->ut_cut.as<uint8_t>();
        rank(c, a, cut, rounds, false, &state, &launches);
    }
    // the layout
    UtgPlace *place = c->ut_read.as<UtgPlace>();
    long long *scan0 = c->ut_scan.as<long long>(), *scan1 = scan0 + (n + 1), *partials = scan1 + (n + 1);
    hipLaunchKernelGGL(utg_place_kernel, dim3(utg_grid(a.n_reads)), dim3(kUtgThreads), 0, c->stream, state, a.n_reads, a.len, a.span, a.flags, cut, place,
                       c->ut_offset.as<long long>(), c->ut_ulen.as<long long>(), c->ut_orient.as<uint8_t>());
    exclusive_scan<UtgStartLoader, 2>(c->stream, UtgStartLoader{place}, (long long)n, partials, ScanOut<2>{{scan0, scan1}});
    const UtgOut out{c->ut_unitig.as<int32_t>(), c->ut_unitig.as<int32_t>() + n, c->ut_order.as<int32_t>(), c->ut_utg[0].as<long long>(),
                     c->ut_utg[1].as<int32_t>(), c->ut_utg[2].as<long long>(), c->ut_utg[3].as<uint8_t>()};
    hipLaunchKernelGGL(utg_emit_kernel, dim3(utg_grid(a.n_reads)), dim3(kUtgThreads), 0, c->stream, place, a.n_reads, c->ut_ulen.as<long long>(), cut,
                       scan0, scan1, out, ctl);
    launches += 4;
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    PHASE(read_ctl(c, ctl, h_ctl, kUtgCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(&part));
    seconds += part;
    if (a.launches) *a.launches = launches;
    if (a.kernel_seconds) *a.kernel_seconds = seconds;
    const unsigned long long *t = h_ctl + kUtgCtlTotals;
    const size_t n_utg = (size_t)t[kUtgUnitigs], placed = n - (size_t)t[kUtgSkipped];
    PHASE(queue_copies(c, {{a.unitig, out.unitig, n * 4}, {a.index, out.index, n * 4}, {a.offset, c->ut_offset.p, n * 8},
                           {a.orient, c->ut_orient.p, n}, {a.order, out.order, placed * 4}, {a.utg_off, out.utg_off, (n_utg + 1) * 8},
                           {a.utg_reads, out.utg_reads, n_utg * 4}, {a.utg_length, out.utg_length, n_utg * 8},
                           {a.utg_circular, out.utg_circular, n_utg}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (a.sum)
        *a.sum = raft_hip_utg_summary{(int64_t)a.n_reads, (int64_t)t[kUtgSkipped], (int64_t)t[kUtgUnitigs], (int64_t)t[kUtgSingletons],
                                      (int64_t)t[kUtgCircular], (int64_t)t[kUtgLongestReads], (int64_t)t[kUtgLongestLength],
                                      (int64_t)t[kUtgTotalLength]};
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_utg_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_unitigs_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, const int32_t *d_partner, const int32_t *d_span,
                            const uint8_t *d_flags, int32_t *unitig, int32_t *index, int64_t *offset, uint8_t *orient, int32_t *order,
                            int64_t *utg_off, int32_t *utg_reads, int64_t *utg_length, uint8_t *utg_circular, raft_hip_utg_summary *sum,
                            int64_t *error_index, double *kernel_seconds, int64_t *launches)
{
    const UtgCall a{n_reads, d_read_len, d_partner, d_span, d_flags, unitig, index, offset, orient, order, utg_off, utg_reads, utg_length,
                    utg_circular, sum, error_index, kernel_seconds, launches};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return utg_run(c, a);
}

// The same from host arrays: the lengths staged through q_len, partner and span through q_col[0] and q_col[1], which no pass uses,
// the flag bytes through ut_flags.
int raft_hip_unitigs_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, const int32_t *partner, const int32_t *span,
                          const uint8_t *flags, int32_t *unitig, int32_t *index, int64_t *offset, uint8_t *orient, int32_t *order,
                          int64_t *utg_off, int32_t *utg_reads, int64_t *utg_length, uint8_t *utg_circular, raft_hip_utg_summary *sum,
                          int64_t *error_index, double *kernel_seconds, int64_t *launches)
{
    UtgCall a{n_reads, read_len, partner, span, flags, unitig, index, offset, orient, order, utg_off, utg_reads, utg_length,
              utg_circular, sum, error_index, kernel_seconds, launches};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_reads > 0) {
        PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
        PHASE(stage_host(c, c->q_col[0], partner, (size_t)n_reads * 2, &a.partner));
        PHASE(stage_host(c, c->q_col[1], span, (size_t)n_reads * 2, &a.span));
        PHASE(stage_host(c, c->ut_flags, flags, (size_t)n_reads, &a.flags));
    }
    return utg_run(c, a);
}

} // extern "C"
