// containment_rule.hpp -- the rule of include/raft_hip_ctn.h as plain functions: the containment views of a record, which of them may
// place a read, the two keys a read's slot takes the maximum of, the clamped place in the parent, and the composition of two places
// on the way to the root.  Integers only, no HIP include: the kernels of containment.hpp use it, and a host compiler alone builds it
// (tests/containment_rule_check.cpp does, under the sanitizers).
#pragma once
#include "ovl_ends_rule.hpp"

namespace raft {

// the bits of a read's flag byte (RAFT_HIP_CTN_* of raft_hip_ctn.h)
constexpr unsigned kCtnHasParent = 1, kCtnParentRev = 2, kCtnRootRev = 4, kCtnUnplacedView = 8, kCtnOrphan = 16;
constexpr int32_t kCtnIdMask = 0x7FFFFFFF;
constexpr int32_t kCtnMaxReads = (1 << 30) - 1;

// A containment view: read r lies in read c, [as, ae) of r aligned with [bs, be) of c.
struct CtnView { int32_t r, c, as, ae, bs, be; };

// the view of a QUERY_CONTAINED record from its query, and of a TARGET_CONTAINED record from its target
RAFT_ENDS_FN CtnView ctn_query_view(int32_t qid, int32_t qs, int32_t qe, int32_t tid, int32_t ts, int32_t te) { return CtnView{qid, tid, qs, qe, ts, te}; }
RAFT_ENDS_FN CtnView ctn_target_view(int32_t qid, int32_t qs, int32_t qe, int32_t tid, int32_t ts, int32_t te) { return CtnView{tid, qid, ts, te, qs, qe}; }

// May c be r's parent?  The longer read, then the smaller id: a strict order over the reads, so the parents form a forest.
RAFT_ENDS_FN bool ctn_acceptable(int32_t lr, int32_t r, int32_t lc, int32_t c) { return lc > lr || (lc == lr && c < r); }

// key1: the longest container, then the smaller id.  0 is "no parent": a container's length is at least 1.
RAFT_ENDS_FN uint64_t ctn_key1(int32_t lc, int32_t c) { return (uint64_t)(uint32_t)lc << 31 | (uint64_t)(uint32_t)(kCtnIdMask - c); }
RAFT_ENDS_FN int32_t ctn_key1_parent(uint64_t key1) { return key1 ? kCtnIdMask - (int32_t)(key1 & (uint64_t)kCtnIdMask) : -1; }

// Where r (length lr) begins in c (length lc >= lr) under a view, on c's forward strand, clamped into [0, lc - lr].
RAFT_ENDS_FN int32_t ctn_pos(int32_t as, int32_t ae, int32_t bs, int32_t lr, int32_t lc, bool rev)
{
    const int64_t raw = rev ? (int64_t)bs - ((int64_t)lr - ae) : (int64_t)bs - as;
    const int64_t hi = (int64_t)lc - lr;
    return (int32_t)(raw < 0 ? 0 : (raw > hi ? hi : raw));
}

RAFT_ENDS_FN int32_t ctn_span(int32_t as, int32_t ae, int32_t bs, int32_t be) { return ae - as < be - bs ? ae - as : be - bs; }

// key2: the longest span, then '-' before '+', then the smaller pos.  0 is "no view": a view's span is at least 1.
RAFT_ENDS_FN uint64_t ctn_key2(int32_t span, bool rev, int32_t pos)
{
    return (uint64_t)(uint32_t)span << 32 | (uint64_t)(rev ? 1u : 0u) << 31 | (uint64_t)(uint32_t)(kCtnIdMask - pos);
}
RAFT_ENDS_FN int32_t ctn_key2_span(uint64_t key2) { return (int32_t)(key2 >> 32); }
RAFT_ENDS_FN bool ctn_key2_rev(uint64_t key2) { return ((key2 >> 31) & 1u) != 0; }
RAFT_ENDS_FN int32_t ctn_key2_pos(uint64_t key2) { return kCtnIdMask - (int32_t)(key2 & (uint64_t)kCtnIdMask); }

// key2 of a view of r in its parent
RAFT_ENDS_FN uint64_t ctn_view_key2(const CtnView &v, int32_t lr, int32_t lc, bool rev)
{
    return ctn_key2(ctn_span(v.as, v.ae, v.bs, v.be), rev, ctn_pos(v.as, v.ae, v.bs, lr, lc, rev));
}

// A place: where a read begins in an ancestor, and whether it lies there reversed.
struct CtnPlace { int32_t pos; bool rev; };

// r (length lr) lies in a (length la) at `in_a`, a lies in an ancestor of its own at `a_in`: where r lies in that ancestor.
// Associative: composing r -> a -> b -> c either way round gives one place (tests/containment_rule_check.cpp walks all strand pairs).
RAFT_ENDS_FN CtnPlace ctn_compose(CtnPlace in_a, int32_t lr, int32_t la, CtnPlace a_in)
{
    return CtnPlace{a_in.rev ? a_in.pos + (la - in_a.pos - lr) : a_in.pos + in_a.pos, in_a.rev != a_in.rev};
}

// second call: where a read (length lr) with root R (length lR) at `in_root` begins on a unitig that holds R at `off`, orientation o
RAFT_ENDS_FN int64_t ctn_unitig_start(int64_t off, bool o, int32_t lR, int32_t root_pos, int32_t lr)
{
    return o ? off + ((int64_t)lR - root_pos - lr) : off + root_pos;
}

RAFT_ENDS_FN int64_t ctn_depth_permille(int64_t placed_bases, int64_t length) { return length == 0 ? 0 : placed_bases * 1000 / length; }

// rounds of pointer jumping for n reads: ceil(log2(max(n, 2)))
RAFT_ENDS_FN int ctn_rounds(int32_t n_reads)
{
    const int64_t n = n_reads < 2 ? 2 : n_reads;
    int k = 0;
    while (((int64_t)1 << k) < n) ++k;
    return k;
}

} // namespace raft
