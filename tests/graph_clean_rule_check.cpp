// graph_clean_rule_check.cpp -- the rule of include/raft_hip_cln.h as raft_amd/csrc/graph_clean_rule.hpp states it, checked on the CPU as
// a program of its own (tests/test_graph_clean_rule.py builds it under the address and undefined-behaviour sanitizers): the weak
// predicate at equality, one span unit below it, at the edge of the 64-bit products and at W = 0 and 1000; the candidate predicate
// at reads == T and T + 1 and with T = 0; "beats" over every pair among a handful of chain records; and what makes an edge bad.
#include "../raft_amd/csrc/graph_clean_rule.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

using namespace raft;

int main()
{
    const int32_t B = 2147483647;
    // ---- weak: span * 1000 < W * m
    CHECK(!cln_weak(1000, 500, 2000));                     // equality: the arc stays
    CHECK(cln_weak(999, 500, 2000));                       // one span unit below it falls
    CHECK(!cln_weak(1001, 500, 2000));
    CHECK(!cln_weak(1, 500, 2) && cln_weak(1, 500, 3));
    for (int32_t m : {1, 2, 999, 1000, 1001, B}) {
        CHECK(!cln_weak(m, 1000, m));                      // the best arc of an end is never weak, whatever W
        CHECK(!cln_weak(m, 0, m) && !cln_weak(1, 0, m));   // W = 0 cuts nothing
        CHECK(m == 1 || cln_weak(m - 1, 1000, m));         // W = 1000 cuts everything below the best
    }
    // the products at the edge of what int32 factors give: 1000 * (2^31 - 1) needs 41 bits
    CHECK(!cln_weak(B, 1000, B) && cln_weak(B - 1, 1000, B) && !cln_weak(B, 999, B));
    CHECK(cln_weak(1, 1, B) && !cln_weak(2147484, 1, B) && cln_weak(2147483, 1, B));      // 2147483 * 1000 < 2^31 - 1 <= 2147484 * 1000
    CHECK(cln_weak(1073741823, 500, B) && !cln_weak(1073741824, 500, B));                 // 2 * span < 2^31 - 1
    // ---- candidate: not circular, exactly one dead terminal, reads <= T
    for (int32_t T : {1, 3, 4, B - 1}) {
        CHECK(cln_candidate(false, 0, 2, T, T) && cln_candidate(false, 2, 0, T, T));       // reads == T
        CHECK(!cln_candidate(false, 0, 2, T + 1, T));                                      // reads == T + 1
        CHECK(!cln_candidate(true, 0, 2, 1, T));
    }
    CHECK(!cln_candidate(false, 0, 1, 1, 0) && !cln_candidate(false, 3, 0, 1, 0));         // T = 0 makes no chain a candidate
    CHECK(cln_candidate(false, 0, 1, 1, 1) && cln_candidate(false, 7, 0, 1, 1));
    CHECK(!cln_candidate(false, 0, 0, 1, 4) && !cln_candidate(false, 1, 1, 1, 4));         // dead at both ends, dead at neither
    CHECK(cln_isolated_short(false, 0, 0, 4, 4) && !cln_isolated_short(false, 0, 0, 5, 4) && !cln_isolated_short(false, 0, 1, 1, 4) &&
          !cln_isolated_short(true, 0, 0, 1, 4) && !cln_isolated_short(false, 0, 0, 1, 0));
    // ---- beats: a strict total order among candidates; a non-candidate beats every candidate
    struct Rec { int32_t reads; int64_t length; int32_t first; };
    const Rec recs[] = {{1, 1000, 7}, {1, 1000, 3}, {1, 1001, 9}, {2, 500, 8}, {2, 500, 1}, {3, 1, 5}, {1, (int64_t)1 << 40, 6}, {B, ((int64_t)1 << 62), 0}};
    const int n = (int)(sizeof recs / sizeof recs[0]);
    for (int a = 0; a < n; ++a) {
        const Rec &x = recs[a];
        CHECK(!cln_beats(true, x.reads, x.length, x.first, x.reads, x.length, x.first));  // irreflexive
        for (int b = 0; b < n; ++b) {
            if (a == b) continue;
            const Rec &y = recs[b];
            const bool xy = cln_beats(true, x.reads, x.length, x.first, y.reads, y.length, y.first);
            const bool yx = cln_beats(true, y.reads, y.length, y.first, x.reads, x.length, x.first);
            CHECK(xy != yx);                                                               // total and antisymmetric: first differs between chains
            CHECK(cln_beats(false, x.reads, x.length, x.first, y.reads, y.length, y.first));
            for (int c = 0; c < n; ++c) {
                const Rec &z = recs[c];
                if (c == a || c == b) continue;
                const bool yz = cln_beats(true, y.reads, y.length, y.first, z.reads, z.length, z.first);
                const bool xz = cln_beats(true, x.reads, x.length, x.first, z.reads, z.length, z.first);
                CHECK(!(xy && yz) || xz);                                                  // transitive
            }
        }
    }
    CHECK(cln_beats(true, 2, 1, 9, 1, 1000000, 0));        // more reads win whatever the length
    CHECK(cln_beats(true, 1, 1001, 9, 1, 1000, 3));        // a tie in reads is broken by the length
    CHECK(cln_beats(true, 1, 1000, 3, 1, 1000, 7) && !cln_beats(true, 1, 1000, 7, 1, 1000, 3));      // a tie in both by the smaller first
    {
        ClnChain d{1, 3, 1000, {6, 7}, 6, 0}, c{1, 7, 1000, {14, 15}, 14, 0};
        CHECK(cln_beats(d, c) && !cln_beats(c, d));
        d.attached = -1; d.reads = 0;                      // (no candidate: it beats whatever its record says)
        CHECK(cln_beats(d, c));
    }
    // ---- a bad edge, as far as the edge alone says
    {
        const int32_t len[4] = {100, 50, -5, 70};
        const uint8_t skip[4] = {0, 0, 0, 9};
        CHECK(cln_edge_ok(4, len, nullptr, 1, 2, 50) && cln_edge_ok(4, len, skip, 2, 1, 1) && cln_edge_ok(4, len, nullptr, 0, 7, 70));
        CHECK(!cln_edge_ok(4, len, nullptr, 1, 2, 51) && !cln_edge_ok(4, len, nullptr, 1, 2, 0) && !cln_edge_ok(4, len, nullptr, 1, 2, -1));
        CHECK(!cln_edge_ok(4, len, nullptr, -1, 2, 5) && !cln_edge_ok(4, len, nullptr, 1, 8, 5) && !cln_edge_ok(4, len, nullptr, 8, 1, 5) &&
              !cln_edge_ok(4, len, nullptr, 1, B, 5) && !cln_edge_ok(4, len, nullptr, -B - 1, 1, 5));
        CHECK(!cln_edge_ok(4, len, nullptr, 2, 3, 5) && !cln_edge_ok(4, len, nullptr, 3, 3, 5));      // one read twice
        CHECK(!cln_edge_ok(4, len, skip, 1, 6, 5) && cln_edge_ok(4, len, nullptr, 1, 6, 5));         // a flagged read
        CHECK(!cln_edge_ok(4, len, nullptr, 1, 4, 1));                                               // a negative length counts as 0
        CHECK(!cln_edge_ok(0, len, nullptr, 0, 0, 1) && !cln_edge_ok((1 << 30) - 1, len, nullptr, B, 0, 1));
    }
    printf("graph_clean_rule_check: ok\n");
    return 0;
}
