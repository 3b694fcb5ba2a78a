// query_host.hpp -- the host side that the queries about a finished pass or a record stream share (engine.hip: cov_histogram,
// read_stats, census; low_cov_lib.hip, ovl_class_lib.hip, frag_ovl_lib.hip, repeat_stats_lib.hip, filter_lib.hip, ovl_ends_lib.hip, best_ovl_lib.hip, unitig_lib.hip): phases, grids, copy tables, the
// staging of a host form, the caller's table or the pass's, the event pair, the control words.  Everything works on a raft_hip_ctx
// and its stream; no helper knows which query calls it -- what differs between them (whether the clears are timed, where a copy
// goes, which totals make the summary) stays with the caller.  The decisions free of HIP are in query_args.hpp; the coverage decode,
// which needs pack.hpp's kernels in the translation unit, is in cov_decode.hpp.
#pragma once
#include "engine_ctx.hpp"
#include "query_args.hpp"

#include <initializer_list>
#include <string>

namespace raft {

// HIP_TRY's companion (engine_ctx.hpp): a step that returns a code of the ABI.  (engine_pipeline.hip has a PHASE of its own, which
// also knows the way out to the one-piece pass; it does not include this header.)
#define PHASE(expr)                                              \
    do {                                                         \
        const int rc_ = (expr);                                  \
        if (rc_ != RAFT_HIP_OK) return rc_;                      \
    } while (0)

// A query refused on the host before any launch: the code, and the context's message naming the call and the reason (raft_hip_last_error).
inline int refuse(raft_hip_ctx *c, int code, const char *who, const char *why)
{
    if (c) c->last_error = std::string(who) + ": " + why;
    return code;
}
constexpr const char *kNoPass = "the context holds no finished pass (none ran, the last one reported an error, or a host-to-host job ran in chunks)";
constexpr const char *kOtherReads = "n_reads is not that of the context's finished pass";
constexpr const char *kBadArgs = "an argument out of range or a missing array";

// What the calls under the rule of ovl_ends_rule.hpp (overlap_ends, best_overlaps) check, in both forms, before anything is staged.
inline int check_ends_rule_call(raft_hip_ctx *c, const char *who, int32_t max_overhang, int32_t min_ratio, int32_t n_reads, const int32_t *read_len,
                                const RecordCols &rec, const uint8_t *strand)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (max_overhang < 0) return refuse(c, RAFT_HIP_ERR_PARAM, who, "max_overhang is negative");
    if (min_ratio < 0 || min_ratio > 1000) return refuse(c, RAFT_HIP_ERR_PARAM, who, "min_ratio_permille outside [0, 1000]");
    if (n_reads < 0) return refuse(c, RAFT_HIP_ERR_PARAM, who, "n_reads is negative");
    if (rec.n_rec < 0) return refuse(c, RAFT_HIP_ERR_PARAM, who, "n_rec is negative");
    if (n_reads > 0 && !read_len) return refuse(c, RAFT_HIP_ERR_PARAM, who, "read_len is missing");
    if (rec.n_rec > 0 && (!record_cols_ok(rec, false, TargetCols::always) || !strand))
        return refuse(c, RAFT_HIP_ERR_PARAM, who, "a missing column (the six and strand)");
    return RAFT_HIP_OK;
}

// blocks of `per_block` items for n of them, one at least and `cap` at most
inline unsigned grid_for(long long n, long long per_block, long long cap)
{
    return (unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, cap));
}

// Rows of a copy table: a destination the caller left NULL, or nothing to copy, is skipped.
struct CopyRow { void *dst; const void *src; size_t bytes; hipMemcpyKind kind = hipMemcpyDeviceToHost; };
inline int queue_copies(raft_hip_ctx *c, std::initializer_list<CopyRow> rows)
{
    for (const CopyRow &j : rows)
        if (j.dst && j.bytes) HIP_TRY(c, hipMemcpyAsync(j.dst, j.src, j.bytes, j.kind, c->stream));
    return RAFT_HIP_OK;
}

// A host array into a staging buffer of the context, *dev then the device copy (of one element at least, so that it is never NULL).
// Callers stage what the caller of the entry point gave: a column left NULL is not staged and stays NULL.
template <class T> int stage_host(raft_hip_ctx *c, DevBuf &buf, const T *src, size_t count, const T **dev)
{
    HIP_TRY(c, buf.ensure(std::max<size_t>(count, 1) * sizeof(T)));
    if (count > 0 && src) HIP_TRY(c, hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *dev = buf.as<T>();
    return RAFT_HIP_OK;
}

// ... the record columns that are there, into six buffers
inline int stage_columns(raft_hip_ctx *c, DevBuf *bufs, RecordCols &r)
{
    for (int k = 0; k < 6; ++k)
        if (r.col[k]) PHASE(stage_host(c, bufs[k], r.col[k], (size_t)r.n_rec, &r.col[k]));
    return RAFT_HIP_OK;
}

// ... the three arrays of a table the caller gave (CsrKind::given)
inline int stage_csr(raft_hip_ctx *c, DevBuf *bufs, CsrArg &a, int32_t n_reads)
{
    PHASE(stage_host(c, bufs[0], a.off, (size_t)n_reads + 1, &a.off));
    PHASE(stage_host(c, bufs[1], a.x, (size_t)a.count, &a.x));
    return stage_host(c, bufs[2], a.y, (size_t)a.count, &a.y);
}

// The device arrays a query reads a table from: the context's own pass (count -1) or what the caller gave.
struct CsrDev { const long long *off; const int32_t *x, *y; long long count; };
inline CsrDev resolve_csr(const CsrArg &a, const DevBuf &own_off, const DevBuf &own_x, const DevBuf &own_y, long long own_count)
{
    if (a.count == -1) return {own_off.as<long long>(), own_x.as<int32_t>(), own_y.as<int32_t>(), own_count};
    return {reinterpret_cast<const long long *>(a.off), a.x, a.y, (long long)a.count};
}

// Device time between start() and stop() on the context's stream (ev_hist0/1, made at the first call that asks for the time).
// Does nothing when the caller of the entry point passed no kernel_seconds.
struct QueryTimer {
    raft_hip_ctx *c;
    bool on;
    QueryTimer(raft_hip_ctx *ctx, const double *kernel_seconds) : c(ctx), on(kernel_seconds != nullptr) {}
    int start()
    {
        if (!on) return RAFT_HIP_OK;
        if (!c->ev_hist0) { HIP_TRY(c, hipEventCreate(&c->ev_hist0)); HIP_TRY(c, hipEventCreate(&c->ev_hist1)); }
        HIP_TRY(c, hipEventRecord(c->ev_hist0, c->stream));
        return RAFT_HIP_OK;
    }
    int stop()
    {
        if (on) HIP_TRY(c, hipEventRecord(c->ev_hist1, c->stream));
        return RAFT_HIP_OK;
    }
    // the last span into *span, once the stream has been waited for
    int seconds(double *span)
    {
        if (!on) return RAFT_HIP_OK;
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_hist0, c->ev_hist1));
        *span = ms * 1e-3;
        return RAFT_HIP_OK;
    }
};

// The control words of a record query: word 0 = the first bad record (all ones: none, the kernels take the minimum), the others count.
inline int clear_ctl(raft_hip_ctx *c, unsigned long long *ctl, int words)
{
    HIP_TRY(c, hipMemsetAsync(ctl, 0xFF, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(ctl + 1, 0, (size_t)(words - 1) * 8, c->stream));
    return RAFT_HIP_OK;
}
// ... queued for the host (valid after the next wait)
inline int read_ctl(raft_hip_ctx *c, const unsigned long long *ctl, unsigned long long *host, int words)
{
    HIP_TRY(c, hipMemcpyAsync(host, ctl, (size_t)words * 8, hipMemcpyDeviceToHost, c->stream));
    return RAFT_HIP_OK;
}
// ... and word 0 as the caller's error_index: -1, or the record with RAFT_HIP_ERR_READ_ID and the query's message
inline int first_bad_record(raft_hip_ctx *c, unsigned long long word, int64_t *error_index, const char *message)
{
    if (word == ~0ull) {
        if (error_index) *error_index = -1;
        return RAFT_HIP_OK;
    }
    if (error_index) *error_index = (int64_t)word;
    c->last_error = message;
    return RAFT_HIP_ERR_READ_ID;
}

// the buffers hold the codes the last pass wrote (a caller that had them re-encoded in another width since holds the int32 array as well)
inline bool pass_holds_codes(const raft_hip_ctx *c)
{
    return (c->pass_width == 1 || c->pass_width == 2) && c->packed_width == c->pass_width;
}

} // namespace raft
