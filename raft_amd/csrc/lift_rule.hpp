// lift_rule.hpp -- the rule of include/raft_hip_lift.h as plain functions: the canonical sides of a record, what one pair of fragment
// rows makes of it, the record put back into query and target order, and the whole rule by brute force over two reads' rows.
// 64-bit integers only, no HIP include: the kernels of lift.hpp use the first three, and a host compiler alone builds it
// (tests/lift_rule_check.cpp does, under the sanitizers; tools/lift_walk.cpp is the brute force over a whole stream).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RAFT_LIFT_FN __host__ __device__ inline
#else
#define RAFT_LIFT_FN inline
#endif

namespace raft {

// The canonical sides of a record: A = [as, ae) on the read with the smaller id, B = [bs, be) on the other; swap: A is the target.
struct LiftSides { int64_t as, ae, bs, be, LA, LB; bool swap; };

// false: the record lifts to nothing (a read with itself, or an empty side)
RAFT_LIFT_FN bool lift_sides(int32_t qid, int32_t qs, int32_t qe, int32_t tid, int32_t ts, int32_t te, LiftSides &s)
{
    if (qid == tid || qe <= qs || te <= ts) return false;
    s.swap = tid < qid;
    s.as = s.swap ? ts : qs; s.ae = s.swap ? te : qe;
    s.bs = s.swap ? qs : ts; s.be = s.swap ? qe : te;
    s.LA = s.ae - s.as; s.LB = s.be - s.bs;
    return true;
}

// row [fb, fe) is touched by the side [s, e)
RAFT_LIFT_FN bool lift_touched(int64_t fb, int64_t fe, int64_t s, int64_t e) { return fe > s && fb < e; }

RAFT_LIFT_FN int64_t lift_min(int64_t a, int64_t b) { return a < b ? a : b; }
RAFT_LIFT_FN int64_t lift_max(int64_t a, int64_t b) { return a > b ? a : b; }
// ceil(x / y), 0 <= x, 0 < y, x + y below 2^63
RAFT_LIFT_FN int64_t lift_ceil_div(int64_t x, int64_t y) { return (x + y - 1) / y; }

// One pair of touched rows, [ab, ae) of A's read and [bb, be) of B's, in coordinates relative to the rows.
struct LiftPair { int32_t a0, a1, b0, b1; };

// false: the pair is dropped under min_len.  Both rows are touched (the caller's business): ua < ub and va < vb.
// The largest product is (vb + 1) * LA <= 2^31 * 2^31.
RAFT_LIFT_FN bool lift_pair(const LiftSides &s, int64_t fb_a, int64_t fe_a, int64_t fb_b, int64_t fe_b, bool rev, int64_t min_len, LiftPair &p)
{
    const int64_t ua = lift_max(0, fb_a - s.as), ub = lift_min(s.LA, fe_a - s.as);
    const int64_t va = rev ? lift_max(0, s.be - fe_b) : lift_max(0, fb_b - s.bs);
    const int64_t vb = rev ? lift_min(s.LB, s.be - fb_b) : lift_min(s.LB, fe_b - s.bs);
    const int64_t u1 = lift_max(ua, lift_ceil_div(va * s.LA, s.LB));
    const int64_t u2 = lift_min(ub, lift_ceil_div((vb + 1) * s.LA, s.LB) - 1);
    if (u2 - u1 < min_len) return false;
    const int64_t v1 = u1 * s.LB / s.LA, v2 = u2 * s.LB / s.LA;
    if (v2 - v1 < min_len) return false;
    p.a0 = (int32_t)(s.as + u1 - fb_a); p.a1 = (int32_t)(s.as + u2 - fb_a);
    p.b0 = (int32_t)(rev ? s.be - v2 - fb_b : s.bs + v1 - fb_b);
    p.b1 = (int32_t)(rev ? s.be - v1 - fb_b : s.bs + v2 - fb_b);
    return true;
}

// The pair of a record that leaves neither of two single rows: ua = va = 0, ub = LA, vb = LB, so u1 = v1 = 0, u2 = LA (the ceiling is
// LA + ceil(LA / LB), above LA) and v2 = LB -- the record itself, shifted, without a division.
RAFT_LIFT_FN bool lift_pair_whole(const LiftSides &s, int64_t fb_a, int64_t fb_b, int64_t min_len, LiftPair &p)
{
    if (s.LA < min_len || s.LB < min_len) return false;
    p.a0 = (int32_t)(s.as - fb_a); p.a1 = (int32_t)(s.ae - fb_a);
    p.b0 = (int32_t)(s.bs - fb_b); p.b1 = (int32_t)(s.be - fb_b);
    return true;
}

// An output in query and target order: rows are global row indices.
struct LiftRecord { int32_t qfrag, qs, qe, tfrag, ts, te; };

RAFT_LIFT_FN LiftRecord lift_record(bool swap, int64_t row_a, int64_t row_b, const LiftPair &p)
{
    if (swap) return LiftRecord{(int32_t)row_b, p.b0, p.b1, (int32_t)row_a, p.a0, p.a1};
    return LiftRecord{(int32_t)row_a, p.a0, p.a1, (int32_t)row_b, p.b0, p.b1};
}

// The whole rule for one record by brute force: every pair of rows of the two reads, i ascending, then j ascending.  off / fb / fe
// are the table; emit(LiftRecord) is called per output.  Returns the outputs; *dropped gains the pairs dropped under min_len.
template <class Emit>
inline int64_t lift_record_brute(const int64_t *off, const int32_t *fb, const int32_t *fe, int32_t qid, int32_t qs, int32_t qe, int32_t tid,
                                 int32_t ts, int32_t te, bool rev, int64_t min_len, int64_t *dropped, Emit emit)
{
    LiftSides s;
    if (!lift_sides(qid, qs, qe, tid, ts, te, s)) return 0;
    const int32_t ra = s.swap ? tid : qid, rb = s.swap ? qid : tid;
    int64_t n = 0;
    for (int64_t i = off[ra]; i < off[ra + 1]; ++i) {
        if (!lift_touched(fb[i], fe[i], s.as, s.ae)) continue;
        for (int64_t j = off[rb]; j < off[rb + 1]; ++j) {
            if (!lift_touched(fb[j], fe[j], s.bs, s.be)) continue;
            LiftPair p;
            if (lift_pair(s, fb[i], fe[i], fb[j], fe[j], rev, min_len, p)) { emit(lift_record(s.swap, i, j, p)); ++n; }
            else if (dropped) ++*dropped;
        }
    }
    return n;
}

} // namespace raft
