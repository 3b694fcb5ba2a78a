// graph_clean_rule.hpp -- the rule of include/raft_hip_cln.h as plain functions: when an edge of the given list is bad, when an arc is
// weak beside the best one of its end, when a chain is a candidate tip and when one chain beats another.  Integers only, no HIP
// include: the kernels of graph_clean.hpp use it, and a host compiler alone builds it (tests/graph_clean_rule_check.cpp does, under
// the sanitizers).
#pragma once
#include <cstdint>
#include "unitig_rule.hpp"

namespace raft {

// the bits of an edge's state byte (RAFT_HIP_CLN_* of raft_hip_cln.h) and a read's state
constexpr int kClnWeakU = 1, kClnWeakW = 2, kClnTip = 4;
constexpr int kClnReadStays = 0, kClnReadTip = 1, kClnReadFlagged = 2;
constexpr int kClnMaxRounds = 64;

// What can be said of edge (u, w, span) without the rest of the list: both nodes in [0, 2 * n_reads), two different reads, neither
// flagged, 1 <= span <= the shorter length.  (That its pair stands at no smaller index is the list's matter: graph_clean.hpp.)
RAFT_ENDS_FN bool cln_edge_ok(int32_t n_reads, const int32_t *len, const uint8_t *skip, int32_t u, int32_t w, int32_t span)
{
    const int64_t n_nodes = 2 * (int64_t)n_reads;
    if (u < 0 || u >= n_nodes || w < 0 || w >= n_nodes) return false;
    const int32_t ru = u >> 1, rw = w >> 1;
    if (ru == rw) return false;
    if (skip && (skip[ru] || skip[rw])) return false;
    const int32_t lu = utg_len(len[ru]), lw = utg_len(len[rw]);
    return span >= 1 && span <= (lu < lw ? lu : lw);
}

// Arc u -> w of span `span` is weak beside m, the greatest span of an arc that leaves u, under W per mille: span * 1000 < W * m, the
// products in 64 bits (span and m are below 2^31, W is at most 1000).
RAFT_ENDS_FN bool cln_weak(int32_t span, int32_t w_permille, int32_t m)
{
    return (int64_t)span * 1000 < (int64_t)w_permille * (int64_t)m;
}

// A chain as the rounds judge it.  attached: the terminal end of a candidate that is not dead, -1 for every other chain.
struct ClnChain {
    int32_t reads;                           // 0: the read is flagged or removed and belongs to no chain
    int32_t first;                           // its smallest read id
    int64_t length;                          // by the layout rule of raft_hip_utg.h
    int32_t term[2];                         // its terminal nodes (where it is not circular)
    int32_t attached;
    int32_t circular;
};
static_assert(sizeof(ClnChain) == 32, "one chain record, one 32-byte line");

// A chain is a candidate: not circular, exactly one terminal end without a live arc, at most T reads.  (T == 0: none is.)
RAFT_ENDS_FN bool cln_candidate(bool circular, int32_t deg_a, int32_t deg_b, int32_t reads, int32_t max_tip_reads)
{
    return !circular && ((deg_a == 0) != (deg_b == 0)) && reads <= max_tip_reads;
}

// D beats candidate C: D is no candidate, or (reads, length, -first) of D is lexicographically greater.
RAFT_ENDS_FN bool cln_beats(bool d_candidate, int32_t d_reads, int64_t d_length, int32_t d_first, int32_t c_reads, int64_t c_length, int32_t c_first)
{
    if (!d_candidate) return true;
    if (d_reads != c_reads) return d_reads > c_reads;
    if (d_length != c_length) return d_length > c_length;
    return d_first < c_first;
}
RAFT_ENDS_FN bool cln_beats(const ClnChain &d, const ClnChain &c)
{
    return cln_beats(d.attached >= 0, d.reads, d.length, d.first, c.reads, c.length, c.first);
}

// A chain that stands alone and is short: both terminal ends dead, at most T reads (the summary's isolated_short).
RAFT_ENDS_FN bool cln_isolated_short(bool circular, int32_t deg_a, int32_t deg_b, int32_t reads, int32_t max_tip_reads)
{
    return !circular && deg_a == 0 && deg_b == 0 && reads <= max_tip_reads;
}

} // namespace raft
