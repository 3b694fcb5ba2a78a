// containment_rule_check.cpp -- the rule of include/raft_hip_ctn.h as raft_amd/csrc/containment_rule.hpp states it, checked on the CPU as
// a program of its own (tests/test_containment_rule.py builds it under the address and undefined-behaviour sanitizers): acceptability at
// equal lengths and ids, both views on both strands, the clamp below 0 and above lc - lr, the order of the two keys at each tie, the
// associativity of the composition over all four strand pairs, the place on a unitig, the round count.
#include "../raft_amd/csrc/containment_rule.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

using namespace raft;

// the bases [0, lr) of a read at `p` in a read of length la, as the interval they cover on that read's forward strand
struct Interval { long long lo, hi; bool rev; };
static Interval cover(CtnPlace p, int32_t lr) { return Interval{p.pos, (long long)p.pos + lr, p.rev}; }

int main()
{
    // acceptability: the longer read, then the smaller id; never both ways round, never a read in itself
    CHECK(ctn_acceptable(5, 1, 6, 2) && ctn_acceptable(5, 2, 6, 1) && !ctn_acceptable(6, 1, 5, 2) && !ctn_acceptable(6, 2, 5, 1));
    CHECK(ctn_acceptable(5, 2, 5, 1) && !ctn_acceptable(5, 1, 5, 2) && !ctn_acceptable(5, 1, 5, 1));
    CHECK(ctn_acceptable(1, 0, 2147483647, kCtnMaxReads - 1) && !ctn_acceptable(2147483647, 0, 1, 1));
    for (int lr = 1; lr <= 4; ++lr)
        for (int lc = 1; lc <= 4; ++lc)
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c)
                    CHECK(!(ctn_acceptable(lr, r, lc, c) && ctn_acceptable(lc, c, lr, r)) && (r == c && lr == lc ? !ctn_acceptable(lr, r, lc, c) : true));
    // the two views of one record: the roles swapped; a record and its mirror give the same views
    {
        const CtnView q = ctn_query_view(3, 10, 20, 8, 30, 41), t = ctn_target_view(3, 10, 20, 8, 30, 41);
        CHECK(q.r == 3 && q.c == 8 && q.as == 10 && q.ae == 20 && q.bs == 30 && q.be == 41);
        CHECK(t.r == 8 && t.c == 3 && t.as == 30 && t.ae == 41 && t.bs == 10 && t.be == 20);
        const CtnView m = ctn_target_view(8, 30, 41, 3, 10, 20);           // the mirror's target view is the record's query view
        CHECK(m.r == q.r && m.c == q.c && m.as == q.as && m.ae == q.ae && m.bs == q.bs && m.be == q.be);
    }
    // key1: the longest container, then the smaller id; 0 is none; the parent comes back out
    CHECK(ctn_key1(6, 9) > ctn_key1(5, 0) && ctn_key1(5, 3) > ctn_key1(5, 4) && ctn_key1(1, kCtnMaxReads) > 0);
    CHECK(ctn_key1_parent(0) == -1 && ctn_key1_parent(ctn_key1(5, 0)) == 0 && ctn_key1_parent(ctn_key1(2147483647, kCtnMaxReads)) == kCtnMaxReads);
    CHECK(ctn_key1(2147483647, 0) > ctn_key1(2147483646, 0) && ctn_key1_parent(ctn_key1(2147483647, 0)) == 0);
    // the place: on '+' the target's start less the query's; on '-' less what the query leaves at its 3' end; clamped into [0, lc - lr]
    CHECK(ctn_pos(0, 50, 30, 50, 100, false) == 30 && ctn_pos(5, 50, 30, 50, 100, false) == 25 && ctn_pos(5, 45, 30, 50, 100, true) == 25);
    CHECK(ctn_pos(0, 50, 30, 50, 100, true) == 30 && ctn_pos(10, 50, 30, 50, 100, true) == 30);
    CHECK(ctn_pos(40, 50, 30, 50, 100, false) == 0 && ctn_pos(0, 10, 30, 50, 100, true) == 0);                  // pos_raw below 0
    CHECK(ctn_pos(0, 50, 60, 50, 100, false) == 50 && ctn_pos(0, 50, 70, 50, 100, true) == 50);                 // ... above lc - lr
    CHECK(ctn_pos(0, 50, 0, 50, 50, false) == 0 && ctn_pos(0, 50, 1, 50, 50, true) == 0);                       // lc == lr: 0 whatever the view
    CHECK(ctn_pos(0, 1, 2147483646, 1, 2147483647, false) == 2147483646 && ctn_pos(2147483646, 2147483647, 0, 2147483647, 2147483647, false) == 0);
    CHECK(ctn_span(0, 50, 30, 81) == 50 && ctn_span(0, 50, 30, 79) == 49);
    // key2: the longest span, then '-' before '+', then the smaller pos; 0 is none; the three come back out
    CHECK(ctn_key2(51, false, 900) > ctn_key2(50, true, 0) && ctn_key2(50, true, 900) > ctn_key2(50, false, 0) && ctn_key2(50, true, 7) > ctn_key2(50, true, 8));
    CHECK(ctn_key2(1, false, kCtnIdMask) > 0 && ctn_key2(50, false, 7) == ctn_key2(50, false, 7));
    for (int32_t span : {1, 50, 2147483647})
        for (int rev = 0; rev < 2; ++rev)
            for (int32_t pos : {0, 7, 2147483646}) {
                const uint64_t k = ctn_key2(span, rev != 0, pos);
                CHECK(ctn_key2_span(k) == span && ctn_key2_rev(k) == (rev != 0) && ctn_key2_pos(k) == pos);
            }
    {
        const CtnView v{1, 0, 5, 45, 30, 70};
        CHECK(ctn_view_key2(v, 50, 100, true) == ctn_key2(40, true, 25) && ctn_view_key2(v, 50, 100, false) == ctn_key2(40, false, 25));
    }
    // the composition: r in a in b in c, all four strand pairs at every step; associative, inside the ancestor, and what the
    // intervals say -- r's bases cover, on c, the image of what they cover on a
    long long walked = 0;
    const int32_t lr = 3, la = 7, lb = 12, lc = 20;
    for (int32_t p1 = 0; p1 <= la - lr; ++p1)
        for (int32_t p2 = 0; p2 <= lb - la; ++p2)
            for (int32_t p3 = 0; p3 <= lc - lb; ++p3)
                for (int s = 0; s < 8; ++s) {
                    const CtnPlace r_a{p1, (s & 1) != 0}, a_b{p2, (s & 2) != 0}, b_c{p3, (s & 4) != 0};
                    const CtnPlace r_b = ctn_compose(r_a, lr, la, a_b), a_c = ctn_compose(a_b, la, lb, b_c);
                    const CtnPlace left = ctn_compose(r_b, lr, lb, b_c), right = ctn_compose(r_a, lr, la, a_c);
                    CHECK(left.pos == right.pos && left.rev == right.rev);
                    CHECK(0 <= r_b.pos && r_b.pos <= lb - lr && 0 <= left.pos && left.pos <= lc - lr);
                    CHECK(left.rev == (((s & 1) != 0) != ((s & 2) != 0) != ((s & 4) != 0)));
                    // by hand: a's base x lies at b's p2 + x on '+', at p2 + la - 1 - x on '-'
                    const Interval on_a = cover(r_a, lr);
                    const long long lo = a_b.rev ? p2 + la - on_a.hi : p2 + on_a.lo;
                    CHECK(r_b.pos == lo);
                    ++walked;
                }
    CHECK(walked == 5 * 6 * 9 * 8);
    // a root composes to itself; a read as long as its parent sits at 0 either way round
    CHECK(ctn_compose(CtnPlace{4, true}, 3, 7, CtnPlace{0, false}).pos == 4 && ctn_compose(CtnPlace{0, false}, 7, 7, CtnPlace{5, true}).pos == 5);
    // on a unitig: forward at the offset plus the place, reversed counted from the root's other end; a root at its own offset
    CHECK(ctn_unitig_start(1000, false, 20, 4, 3) == 1004 && ctn_unitig_start(1000, true, 20, 4, 3) == 1013);
    CHECK(ctn_unitig_start(1000, false, 20, 0, 20) == 1000 && ctn_unitig_start(1000, true, 20, 0, 20) == 1000);
    CHECK(ctn_unitig_start(9000000000LL, true, 2147483647, 0, 1) == 9000000000LL + 2147483646);
    CHECK(ctn_depth_permille(0, 0) == 0 && ctn_depth_permille(5, 0) == 0 && ctn_depth_permille(2999, 1000) == 2999 && ctn_depth_permille(2999, 2000) == 1499);
    // rounds: ceil(log2(max(n, 2)))
    CHECK(ctn_rounds(0) == 1 && ctn_rounds(1) == 1 && ctn_rounds(2) == 1 && ctn_rounds(3) == 2 && ctn_rounds(4) == 2 && ctn_rounds(5) == 3);
    CHECK(ctn_rounds(1024) == 10 && ctn_rounds(1025) == 11 && ctn_rounds(kCtnMaxReads) == 30);
    printf("containment_rule_check: ok\n");
    return 0;
}
