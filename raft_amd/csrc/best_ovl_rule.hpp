// best_ovl_rule.hpp -- the rule of include/raft_hip_best.h as plain functions: the 64-bit key of a candidate for a read end's best
// overlap, what a key says, and the partner's end.  Integers only, no HIP include: the kernels of best_ovl.hpp use it, and a host
// compiler alone builds it (tests/best_ovl_rule_check.cpp does, under the sanitizers).
#pragma once
#include <cstdint>
#include "ovl_ends_rule.hpp"

namespace raft {

constexpr int kBestSpanShift = 33, kBestPartnerShift = 2, kBestRevShift = 1;
constexpr uint64_t kBestPartnerMask = 0x7FFFFFFFull;
// the bits of a read's flag byte (RAFT_HIP_BEST_* of raft_hip_best.h)
constexpr int kBestRev5 = 1, kBestMutual5 = 2, kBestRev3 = 4, kBestMutual3 = 8, kBestSkipped = 16;

// The key of a candidate: the greater key wins -- the longer span, then the smaller partner id, then '-' before '+'.  span >= 1 (a
// valid record's), 0 <= other < 2^31 - 1; a key is never 0, which stands for "no best overlap".
RAFT_ENDS_FN uint64_t best_pack(int32_t span, int32_t other, bool rev)
{
    return (uint64_t)(uint32_t)span << kBestSpanShift | (kBestPartnerMask - (uint64_t)(uint32_t)other) << kBestPartnerShift |
           (uint64_t)(rev ? 1 : 0) << kBestRevShift;
}

RAFT_ENDS_FN int32_t best_span(uint64_t key) { return (int32_t)(key >> kBestSpanShift); }
RAFT_ENDS_FN int32_t best_partner(uint64_t key) { return (int32_t)(kBestPartnerMask - ((key >> kBestPartnerShift) & kBestPartnerMask)); }
RAFT_ENDS_FN bool best_rev(uint64_t key) { return ((key >> kBestRevShift) & 1) != 0; }

// The end of the partner that an overlap at end E (0 = 5', 1 = 3') of a read meets: the other end on '+', the same end on '-'.
RAFT_ENDS_FN int best_partner_end(int end, bool rev) { return rev ? end : 1 - end; }

// The end of the viewing read a kind is a dovetail at: 0 for kEndQuery5, 1 for kEndQuery3, -1 for every other kind.
RAFT_ENDS_FN int best_end_of(int kind) { return kind == kEndQuery5 ? 0 : kind == kEndQuery3 ? 1 : -1; }

// Slot (r, E) holds `mine`; `theirs` is what slot (partner, partner end) holds.  Mutual: that slot's best overlap leads back to (r, E).
RAFT_ENDS_FN bool best_mutual(int32_t r, int end, uint64_t mine, uint64_t theirs)
{
    if (mine == 0 || theirs == 0) return false;
    return best_partner(theirs) == r && best_partner_end(best_partner_end(end, best_rev(mine)), best_rev(theirs)) == end;
}

} // namespace raft
