// string_graph_rule.hpp -- the rule of include/raft_hip_sg.h as plain functions: the arc a dovetail view gives, the key that chooses
// one arc per (u, w), and when two arcs of a row make a third reducible.  Integers only, no HIP include: the kernels of
// string_graph.hpp use it, and a host compiler alone builds it (tests/string_graph_rule_check.cpp does, under the sanitizers).
#pragma once
#include <cstdint>
#include "best_ovl_rule.hpp"

namespace raft {

// the bits of an edge's flag byte (RAFT_HIP_SG_EDGE_* of raft_hip_sg.h)
constexpr int kSgRedFromU = 1, kSgRedFromW = 2, kSgUnpaired = 4;

// An arc: from node u = 2 * me + E to node w = 2 * other + E'; ext is what the other read adds beyond end E of me, back what me
// keeps beyond the other read's far end, span the overlap.
struct SgArc { int32_t u, w, ext, back, span; };

// The arc of a view -- the record (me qs qe other ts te rev) between reads of lengths lq and lt as `me` sees it, of kind `kind` under
// ends_kind.  false: the kind is no dovetail and *a is left alone.  For a dovetail kind ext >= 1 and back >= 1: kEndQuery3 is
// q5 > t5 with q3 < t3 (neither read lies within the other), kEndQuery5 the same with the ends exchanged.
RAFT_ENDS_FN bool sg_view_arc(int kind, int32_t me, int32_t qs, int32_t qe, int32_t lq, int32_t other, int32_t ts, int32_t te, int32_t lt, bool rev, SgArc *a)
{
    const int end = best_end_of(kind);
    if (end < 0) return false;
    const int32_t q5 = qs, q3 = lq - qe, t5 = rev ? lt - te : ts, t3 = rev ? ts : lt - te;
    a->u = 2 * me + end;
    a->w = 2 * other + best_partner_end(end, rev);
    a->ext = end ? t3 - q3 : t5 - q5;
    a->back = end ? q5 - t5 : q3 - t3;
    a->span = qe - qs < te - ts ? qe - qs : te - ts;
    return true;
}

// The twin of an arc: the same overlap as the other read's end sees it.
RAFT_ENDS_FN SgArc sg_twin(const SgArc &a) { return SgArc{a.w, a.u, a.back, a.ext, a.span}; }

// The key that chooses among the arcs with one (u, w): (span, -ext_lo, -ext_hi), ext_lo the ext of the direction that leaves the read
// with the smaller id.  An arc and its twin have the same key.
struct SgKey { int32_t span, ext_lo, ext_hi; };

RAFT_ENDS_FN SgKey sg_key(int32_t u, int32_t w, int32_t ext, int32_t back, int32_t span)
{
    const bool u_low = (u >> 1) < (w >> 1);
    return SgKey{span, u_low ? ext : back, u_low ? back : ext};
}

// a stands before b: the greater key wins -- the longer span, then the smaller ext_lo, then the smaller ext_hi
RAFT_ENDS_FN bool sg_key_wins(const SgKey &a, const SgKey &b)
{
    if (a.span != b.span) return a.span > b.span;
    if (a.ext_lo != b.ext_lo) return a.ext_lo < b.ext_lo;
    return a.ext_hi < b.ext_hi;
}

// Arc u -> w (ext_uw) is reducible over u -> v (ext_uv) and v ^ 1 -> w (ext_vw) -- the caller has found both and knows v != w --
// when u -> v is strictly nearer and the path's length is that of the arc within fuzz Z >= 0, on either side.  The sum is taken in
// 64 bits: each ext is below 2^31.
RAFT_ENDS_FN bool sg_reducible(int32_t ext_uv, int32_t ext_vw, int32_t ext_uw, int32_t fuzz)
{
    if (!(ext_uv < ext_uw)) return false;
    const int64_t d = (int64_t)ext_uv + ext_vw - ext_uw;
    return (d < 0 ? -d : d) <= (int64_t)fuzz;
}

} // namespace raft
