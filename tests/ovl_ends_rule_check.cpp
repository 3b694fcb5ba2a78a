// ovl_ends_rule_check.cpp -- the rule of include/raft_hip_end.h as raft_amd/csrc/ovl_ends_rule.hpp states it, checked on the CPU as a
// program of its own (tests/test_ovl_ends_rule.py builds it under the address and undefined-behaviour sanitizers): the mirror
// property over a small universe, a table of cases worked out by hand, and 64-bit safety at coordinates near INT32_MAX.
#include "../raft_amd/csrc/ovl_ends_rule.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

using namespace raft;

// the kind of (qid qs qe tid ts te rev) between reads of lengths lq and lt
static int K(int qid, int qs, int qe, int lq, int tid, int ts, int te, int lt, bool rev, int H, int F)
{
    return ends_kind(qid, qs, qe, lq, tid, ts, te, lt, rev, H, F);
}

// Every record over lengths 1..6 -- coordinates from 0 to one past the length, so that invalid ones are among them --, both strands,
// both orders of the two ids and a read against itself: the kind of the mirror is the kind under the target's view.
static long long mirror_universe()
{
    long long n = 0, by_kind[kEndKinds] = {};
    const int Hs[] = {0, 1, 2}, Fs[] = {0, 500, 800, 1000};
    const int ids[][2] = {{0, 1}, {1, 0}, {0, 0}};
    for (int lq = 1; lq <= 6; ++lq)
        for (int lt = 1; lt <= 6; ++lt)
            for (const auto &id : ids) {
                if (id[0] == id[1] && lq != lt) continue;          // (a read has one length)
                for (int qs = 0; qs <= lq + 1; ++qs)
                    for (int qe = 0; qe <= lq + 1; ++qe)
                        for (int ts = 0; ts <= lt + 1; ++ts)
                            for (int te = 0; te <= lt + 1; ++te)
                                for (int rev = 0; rev < 2; ++rev)
                                    for (int H : Hs)
                                        for (int F : Fs) {
                                            const int k = K(id[0], qs, qe, lq, id[1], ts, te, lt, rev != 0, H, F);
                                            const int m = K(id[1], ts, te, lt, id[0], qs, qe, lq, rev != 0, H, F);
                                            CHECK(k >= 0 && k < kEndKinds);
                                            CHECK(m == ends_target_view(k, rev != 0));
                                            CHECK(ends_target_view(ends_target_view(k, rev != 0), rev != 0) == k);
                                            const bool valid = 0 <= qs && qs < qe && qe <= lq && 0 <= ts && ts < te && te <= lt;
                                            CHECK((k == kEndInvalid) == !valid);
                                            CHECK((k == kEndSelf) == (valid && id[0] == id[1]));
                                            ++by_kind[k];
                                            ++n;
                                        }
            }
    for (int k = 0; k < kEndKinds; ++k) CHECK(by_kind[k] > 0);     // (the universe holds every kind)
    return n;
}

static void hand_table()
{
    // e5 == H passes, e5 == H + 1 is internal (F = 0: the ratio never objects)
    CHECK(K(0, 100, 10000, 10000, 1, 200, 9950, 10000, false, 100, 0) == kEndQueryContained);   // q5 100 <= t5 200, q3 0 <= t3 50
    CHECK(K(0, 101, 10000, 10000, 1, 200, 9950, 10000, false, 100, 0) == kEndInternal);
    CHECK(K(0, 101, 10000, 10000, 1, 200, 9950, 10000, false, 101, 0) == kEndQueryContained);
    // ... and e3 the same: q3 = 100 / 101 against t3 = 300
    CHECK(K(0, 0, 9900, 10000, 1, 50, 9700, 10000, false, 100, 0) == kEndQueryContained);
    CHECK(K(0, 0, 9899, 10000, 1, 50, 9700, 10000, false, 100, 0) == kEndInternal);
    // the ratio exactly at F: span 800, e5 100, e3 100 -> 800 * 1000 == 800 * 1000; one base less of span: internal
    CHECK(K(0, 100, 900, 2000, 1, 100, 900, 1000, false, 1000, 800) == kEndTargetContained);     // q5 100 >= t5 100, q3 1100 >= t3 100
    CHECK(K(0, 100, 899, 2000, 1, 100, 899, 1000, false, 1000, 800) == kEndInternal);            // 799000 < 800 * (799 + 100 + 101)
    CHECK(K(0, 100, 899, 2000, 1, 100, 899, 1000, false, 1000, 799) == kEndTargetContained);
    // span is the shorter side: 800 on the query, 900 on the target
    CHECK(K(0, 100, 900, 2000, 1, 100, 1000, 1100, false, 1000, 800) == kEndTargetContained);
    CHECK(K(0, 100, 899, 2000, 1, 100, 1000, 1100, false, 1000, 800) == kEndInternal);
    // both ties: equal overhangs at both ends -- the shorter read is contained, then the read with the larger id
    CHECK(K(0, 10, 990, 1000, 1, 10, 1190, 1200, false, 1000, 800) == kEndQueryContained);
    CHECK(K(0, 10, 1190, 1200, 1, 10, 990, 1000, false, 1000, 800) == kEndTargetContained);
    CHECK(K(0, 10, 990, 1000, 1, 10, 990, 1000, false, 1000, 800) == kEndTargetContained);
    CHECK(K(1, 10, 990, 1000, 0, 10, 990, 1000, false, 1000, 800) == kEndQueryContained);
    CHECK(K(0, 10, 990, 1000, 1, 10, 990, 1000, true, 1000, 800) == kEndTargetContained);
    // both strands of each dovetail
    CHECK(K(0, 6000, 10000, 10000, 1, 0, 4000, 10000, false, 1000, 800) == kEndQuery3);          // q5 6000 > t5 0, q3 0 < t3 6000
    CHECK(K(0, 6000, 10000, 10000, 1, 6000, 10000, 10000, true, 1000, 800) == kEndQuery3);       // '-': t5 = lt - te = 0, t3 = ts = 6000
    CHECK(K(0, 0, 4000, 10000, 1, 6000, 10000, 10000, false, 1000, 800) == kEndQuery5);          // q5 0 < t5 6000, q3 6000 > t3 0
    CHECK(K(0, 0, 4000, 10000, 1, 0, 4000, 10000, true, 1000, 800) == kEndQuery5);               // '-': t5 = 6000, t3 = 0
    // ... which the strand alone turns into internal matches: the same coordinates on the other strand
    CHECK(K(0, 6000, 10000, 10000, 1, 0, 4000, 10000, true, 1000, 800) == kEndInternal);
    CHECK(K(0, 0, 4000, 10000, 1, 0, 4000, 10000, false, 1000, 800) == kEndInternal);
    // invalid coordinates; self
    CHECK(K(0, 500, 500, 1000, 1, 0, 500, 1000, false, 1000, 800) == kEndInvalid);               // qs == qe
    CHECK(K(0, 0, 500, 1000, 1, 600, 1001, 1000, false, 1000, 800) == kEndInvalid);              // te > lt
    CHECK(K(0, -1, 500, 1000, 1, 0, 500, 1000, false, 1000, 800) == kEndInvalid);
    CHECK(K(0, 0, 1001, 1000, 1, 0, 500, 1000, false, 1000, 800) == kEndInvalid);
    CHECK(K(0, 0, 500, 1000, 1, 700, 600, 1000, false, 1000, 800) == kEndInvalid);
    CHECK(K(3, 0, 500, 1000, 3, 500, 1000, 1000, false, 1000, 800) == kEndSelf);
    CHECK(K(3, 0, 500, 1000, 3, 500, 1000, 1000, true, 0, 1000) == kEndSelf);
    CHECK(K(3, 0, 0, 1000, 3, 500, 1000, 1000, false, 1000, 800) == kEndInvalid);                // (invalid goes first)
    // the target's view, the slots and the status
    CHECK(ends_target_view(kEndQueryContained, false) == kEndTargetContained && ends_target_view(kEndTargetContained, true) == kEndQueryContained);
    CHECK(ends_target_view(kEndQuery3, false) == kEndQuery5 && ends_target_view(kEndQuery5, false) == kEndQuery3);
    CHECK(ends_target_view(kEndQuery3, true) == kEndQuery3 && ends_target_view(kEndQuery5, true) == kEndQuery5);
    for (int k : {kEndInvalid, kEndInternal, kEndSelf}) CHECK(ends_target_view(k, false) == k && ends_target_view(k, true) == k);
    CHECK(ends_count_slot(kEndInvalid) == -1 && ends_count_slot(kEndSelf) == -1 && ends_count_slot(7) == -1 && ends_count_slot(-1) == -1);
    CHECK(ends_count_slot(kEndInternal) == 0 && ends_count_slot(kEndQueryContained) == 1 && ends_count_slot(kEndTargetContained) == 2);
    CHECK(ends_count_slot(kEndQuery5) == 3 && ends_count_slot(kEndQuery3) == 4);
    CHECK(ends_status(1, 5, 5) == kEndContained && ends_status(2, 0, 0) == kEndContained);
    CHECK(ends_status(0, 0, 0) == kEndIsolated && ends_status(0, 0, 3) == kEndDead5 && ends_status(0, 3, 0) == kEndDead3 && ends_status(0, 1, 1) == kEndLinked);
}

static void near_int32_max()
{
    const int M = 2147483647;
    // span * 1000 and F * (span + e5 + e3) beyond 32 bits
    CHECK(K(0, 0, M, M, 1, 0, M, M, false, M, 1000) == kEndTargetContained);
    CHECK(K(1, 0, M, M, 0, 0, M, M, true, 0, 1000) == kEndQueryContained);
    CHECK(K(0, M - 1, M, M, 1, 0, 1, M, false, M, 1000) == kEndQuery3);
    CHECK(K(0, 0, 1, M, 1, M - 1, M, M, false, 0, 1000) == kEndQuery5);
    CHECK(K(0, M - 1, M, M, 1, M - 1, M, M, true, 0, 1000) == kEndQuery3);
    // span + e5 + e3 == INT32_MAX exactly
    CHECK(K(0, M - 2, M - 1, M, 1, M - 2, M - 1, M, false, M, 1000) == kEndInternal);
    CHECK(K(0, M - 2, M - 1, M, 1, M - 2, M - 1, M, false, M, 0) == kEndTargetContained);
    CHECK(K(0, M - 2, M - 1, M, 1, M - 2, M - 1, M, false, M - 3, 0) == kEndInternal);           // e5 = M - 2 > H
    CHECK(K(0, M - 2, M - 1, M, 1, M - 2, M - 1, M, false, M - 2, 0) == kEndTargetContained);
    // lt - te and lq - qe at the extremes
    CHECK(K(0, 0, 1, M, 1, 0, 1, M, true, M, 0) == kEndQuery5);                                  // q5 0, q3 M - 1; t5 M - 1, t3 0
    CHECK(K(0, 0, 1, M, 1, 0, 1, M, true, M, 1) == kEndQuery5);                                  // e5 = e3 = 0: span * 1000 >= span
    CHECK(K(0, 0, 1, M, 1, 0, 1, 1, false, M, 1000) == kEndTargetContained);
    CHECK(K(0, 0, M, M, 1, 0, M - 1, M, false, 0, 1000) == kEndQueryContained);                  // q3 0 <= t3 1, and (M - 1) * 1000 on both sides
}

int main()
{
    const long long n = mirror_universe();
    hand_table();
    near_int32_max();
    printf("ovl_ends_rule_check: ok (%lld records)\n", n);
    return 0;
}
