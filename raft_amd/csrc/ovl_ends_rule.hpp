// ovl_ends_rule.hpp -- the rule of include/raft_hip_end.h as plain functions: what kind of overlap a record is, the same record as its
// target sees it, which of a read's five counts it adds to, and a read's status from its counts.  Integers only, no HIP include: the
// kernels of ovl_ends.hpp use it, and a host compiler alone builds it (tests/ovl_ends_rule_check.cpp does, under the sanitizers).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RAFT_ENDS_FN __host__ __device__ inline
#else
#define RAFT_ENDS_FN inline
#endif

namespace raft {

// the kinds (RAFT_HIP_END_* of raft_hip_end.h) and the statuses (RAFT_HIP_END_READ_*)
constexpr int kEndInvalid = 0, kEndInternal = 1, kEndQueryContained = 2, kEndTargetContained = 3, kEndQuery3 = 4, kEndQuery5 = 5, kEndSelf = 6;
constexpr int kEndKinds = 7;
constexpr int kEndLinked = 0, kEndContained = 1, kEndIsolated = 2, kEndDead5 = 3, kEndDead3 = 4;
constexpr int kEndStatuses = 5;
constexpr int kEndCounts = 5;         // a read's row: internal, contained_in, contains, end5, end3

// The kind of the record (qid qs qe tid ts te rev) between reads of lengths lq and lt, under H = max_overhang >= 0 and
// F = min_ratio_permille in [0, 1000].  Every sum stays below 2^31 once the coordinates are in range (span + e5 + e3 <= lq); the two
// products are taken in 64 bits.
RAFT_ENDS_FN int ends_kind(int32_t qid, int32_t qs, int32_t qe, int32_t lq, int32_t tid, int32_t ts, int32_t te, int32_t lt, bool rev, int32_t H, int32_t F)
{
    if (!(0 <= qs && qs < qe && qe <= lq && 0 <= ts && ts < te && te <= lt)) return kEndInvalid;
    if (qid == tid) return kEndSelf;
    const int32_t q5 = qs, q3 = lq - qe, t5 = rev ? lt - te : ts, t3 = rev ? ts : lt - te;
    const int32_t e5 = q5 < t5 ? q5 : t5, e3 = q3 < t3 ? q3 : t3;
    const int32_t span = qe - qs < te - ts ? qe - qs : te - ts;
    if (e5 > H || e3 > H || (int64_t)span * 1000 < (int64_t)F * ((int64_t)span + e5 + e3)) return kEndInternal;
    const bool qin = q5 <= t5 && q3 <= t3, tin = q5 >= t5 && q3 >= t3;
    if (qin && tin) {                 // equal overhangs on both ends: the shorter read is the contained one, then the one with the larger id
        const bool query = lq != lt ? lq < lt : qid > tid;
        return query ? kEndQueryContained : kEndTargetContained;
    }
    if (qin) return kEndQueryContained;
    if (tin) return kEndTargetContained;
    return q5 > t5 ? kEndQuery3 : kEndQuery5;
}

// The kind of the same record as its target sees it: the kind of the mirror (tid ts te qid qs qe rev).
RAFT_ENDS_FN int ends_target_view(int kind, bool rev)
{
    if (kind == kEndQueryContained) return kEndTargetContained;
    if (kind == kEndTargetContained) return kEndQueryContained;
    if (!rev && kind == kEndQuery3) return kEndQuery5;
    if (!rev && kind == kEndQuery5) return kEndQuery3;
    return kind;
}

// Which count of the viewing read's row a kind adds to: internal 0, contained_in 1, contains 2, end5 3, end3 4; -1: none.
RAFT_ENDS_FN int ends_count_slot(int kind)
{
    if (kind < kEndInternal || kind > kEndQuery5) return -1;
    return kind <= kEndTargetContained ? kind - 1 : 8 - kind;
}

RAFT_ENDS_FN int ends_status(int32_t contained_in, int32_t end5, int32_t end3)
{
    if (contained_in > 0) return kEndContained;
    if (end5 == 0 && end3 == 0) return kEndIsolated;
    if (end5 == 0) return kEndDead5;
    if (end3 == 0) return kEndDead3;
    return kEndLinked;
}

} // namespace raft
