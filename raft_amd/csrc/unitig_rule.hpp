// unitig_rule.hpp -- the rule of include/raft_hip_utg.h as plain functions: the half-edges of the best overlap graph, their successor
// and weight, and the consistency a table of best overlaps must have before anything walks it.  Integers only, no HIP include: the
// kernels of unitig.hpp use it, and a host compiler alone builds it (tests/unitig_rule_check.cpp does, under the sanitizers).
#pragma once
#include <cstdint>
#include "best_ovl_rule.hpp"

namespace raft {

constexpr int32_t kUtgNil = -1;                          // no successor
constexpr int32_t kUtgMaxReads = (1 << 30) - 1;          // half-edge ids are int32

// Half-edge h = 2 * r + E: the walk leaves read r through end E (0 = 5', 1 = 3').
RAFT_ENDS_FN int32_t utg_half(int32_t r, int end) { return 2 * r + end; }
RAFT_ENDS_FN int32_t utg_read(int32_t h) { return h >> 1; }
RAFT_ENDS_FN int utg_end(int32_t h) { return h & 1; }
RAFT_ENDS_FN int32_t utg_twin(int32_t h) { return h ^ 1; }

// what a flag byte (RAFT_HIP_BEST_*) says about end E
RAFT_ENDS_FN bool utg_mutual(unsigned flags, int end) { return ((flags >> (2 * end)) & (unsigned)kBestMutual5) != 0; }
RAFT_ENDS_FN bool utg_rev(unsigned flags, int end) { return ((flags >> (2 * end)) & (unsigned)kBestRev5) != 0; }
RAFT_ENDS_FN bool utg_skipped(unsigned flags) { return (flags & (unsigned)kBestSkipped) != 0; }
RAFT_ENDS_FN int32_t utg_len(int32_t len) { return len < 0 ? 0 : len; }

// The consistency of end (r, E): true if the end has no MUTUAL bit (it is no edge and nothing of it is looked at) or if every
// condition of the header holds.  The conditions are symmetric in the two ends of an edge, so (r, E) passes iff (p, E') does.
RAFT_ENDS_FN bool utg_end_ok(int32_t n_reads, const int32_t *len, const int32_t *partner, const int32_t *span, const uint8_t *flags, int32_t r,
                             int end)
{
    const unsigned fr = flags[r];
    if (!utg_mutual(fr, end)) return true;
    if (utg_skipped(fr)) return false;
    const int32_t p = partner[2 * (int64_t)r + end];
    if (p < 0 || p >= n_reads || p == r) return false;
    const unsigned fp = flags[p];
    if (utg_skipped(fp)) return false;
    const bool rev = utg_rev(fr, end);
    const int pe = best_partner_end(end, rev);
    if (!utg_mutual(fp, pe) || utg_rev(fp, pe) != rev) return false;
    if (partner[2 * (int64_t)p + pe] != r) return false;
    const int32_t s = span[2 * (int64_t)r + end];
    if (s != span[2 * (int64_t)p + pe]) return false;
    const int32_t lr = utg_len(len[r]), lp = utg_len(len[p]);
    return s >= 1 && s <= (lr < lp ? lr : lp);
}

// succ(h) of a consistent table: where the walk that leaves r through E leaves the partner (it enters p at E' and leaves at the
// other end), or kUtgNil for an end that is not mutual.
RAFT_ENDS_FN int32_t utg_succ(const int32_t *partner, const uint8_t *flags, int32_t r, int end)
{
    const unsigned fr = flags[r];
    if (!utg_mutual(fr, end)) return kUtgNil;
    return utg_half(partner[2 * (int64_t)r + end], 1 - best_partner_end(end, utg_rev(fr, end)));
}

// w(h) of a mutual end: what the step adds to the layout, the partner's length less the overlap.
RAFT_ENDS_FN int64_t utg_weight(const int32_t *len, const int32_t *partner, const int32_t *span, int32_t r, int end)
{
    return (int64_t)utg_len(len[partner[2 * (int64_t)r + end]]) - (int64_t)span[2 * (int64_t)r + end];
}

// ceil(log2(2 * n_reads)): the rounds of pointer jumping after which every walk has ended or gone round its cycle (0 for no reads)
inline int utg_rounds(int32_t n_reads)
{
    int rounds = 0;
    while (((int64_t)1 << rounds) < 2 * (int64_t)n_reads) ++rounds;
    return rounds;
}

} // namespace raft
