// string_graph_rule_check.cpp -- the rule of include/raft_hip_sg.h as raft_amd/csrc/string_graph_rule.hpp states it, checked on the CPU
// as a program of its own (tests/test_string_graph_rule.py builds it under the address and undefined-behaviour sanitizers): over an
// exhaustive small grid of coordinates, lengths and both strands that every dovetail view gives an arc with ext >= 1 and back >= 1,
// that a record's two views give twin arcs, that the key is the same for an arc and its twin; and the reducible predicate at the
// fuzz, one beyond it on either side, at a tie in ext and at the extremes of int32.
#include "../raft_amd/csrc/string_graph_rule.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

using namespace raft;

static bool same(const SgArc &a, const SgArc &b) { return a.u == b.u && a.w == b.w && a.ext == b.ext && a.back == b.back && a.span == b.span; }

// every record between read 3 (length lq) and read 8 (length lt), either way round, on both strands
static long long grid()
{
    long long arcs = 0, others = 0, at5 = 0, at3 = 0;
    for (int lq = 1; lq <= 6; ++lq)
        for (int lt = 1; lt <= 6; ++lt)
            for (int H : {0, 1, 6})
                for (int F : {0, 800, 1000})
                    for (int way = 0; way < 2; ++way)
                        for (int qs = 0; qs < lq; ++qs)
                            for (int qe = qs + 1; qe <= lq; ++qe)
                                for (int ts = 0; ts < lt; ++ts)
                                    for (int te = ts + 1; te <= lt; ++te)
                                        for (int r = 0; r < 2; ++r) {
                                            const bool rev = r != 0;
                                            const int q = way ? 8 : 3, t = way ? 3 : 8;
                                            const int kind = ends_kind(q, qs, qe, lq, t, ts, te, lt, rev, H, F);
                                            // the mirror's kind is the target's view of this one (ovl_ends_rule_check proves it; once more here)
                                            const int mirror = ends_kind(t, ts, te, lt, q, qs, qe, lq, rev, H, F);
                                            CHECK(mirror == ends_target_view(kind, rev));
                                            SgArc a{-1, -1, -1, -1, -1}, b{-1, -1, -1, -1, -1};
                                            const bool has = sg_view_arc(kind, q, qs, qe, lq, t, ts, te, lt, rev, &a);
                                            const bool twin = sg_view_arc(mirror, t, ts, te, lt, q, qs, qe, lq, rev, &b);
                                            CHECK(has == (kind == kEndQuery3 || kind == kEndQuery5) && has == twin);
                                            if (!has) {
                                                CHECK(a.u == -1 && a.span == -1 && b.u == -1);       // (left alone)
                                                ++others;
                                                continue;
                                            }
                                            ++arcs;
                                            CHECK(a.ext >= 1 && a.back >= 1 && b.ext >= 1 && b.back >= 1);
                                            CHECK(a.span == (qe - qs < te - ts ? qe - qs : te - ts) && a.span >= 1);
                                            const int end = kind == kEndQuery3 ? 1 : 0;
                                            CHECK(a.u == 2 * q + end && a.w == 2 * t + (rev ? end : 1 - end));
                                            CHECK((a.u >> 1) == q && (a.w >> 1) == t && (a.u ^ 1) >> 1 == q);
                                            (end ? at3 : at5) += 1;
                                            // ext and back against the overhangs written out
                                            const int q5 = qs, q3 = lq - qe, t5 = rev ? lt - te : ts, t3 = rev ? ts : lt - te;
                                            CHECK(end ? (a.ext == t3 - q3 && a.back == q5 - t5) : (a.ext == t5 - q5 && a.back == q3 - t3));
                                            CHECK(a.ext <= lt && a.back <= lq);
                                            // the two views are twins, and the twin of the twin is the arc
                                            CHECK(same(b, sg_twin(a)) && same(a, sg_twin(b)) && same(a, sg_twin(sg_twin(a))));
                                            // the key is the same for both, whichever read has the smaller id
                                            const SgKey ka = sg_key(a.u, a.w, a.ext, a.back, a.span), kb = sg_key(b.u, b.w, b.ext, b.back, b.span);
                                            CHECK(ka.span == kb.span && ka.ext_lo == kb.ext_lo && ka.ext_hi == kb.ext_hi);
                                            CHECK(ka.ext_lo == (q < t ? a.ext : a.back) && ka.ext_hi == (q < t ? a.back : a.ext));
                                            CHECK(!sg_key_wins(ka, kb) && !sg_key_wins(kb, ka));
                                        }
    CHECK(arcs > 0 && others > 0 && at5 > 0 && at3 > 0);   // (the grid holds what it is about)
    return arcs;
}

static void keys()
{
    const SgKey k{100, 7, 9};
    CHECK(sg_key_wins(SgKey{101, 8, 10}, k) && !sg_key_wins(k, SgKey{101, 8, 10}));       // the longer span
    CHECK(sg_key_wins(SgKey{100, 6, 99}, k) && !sg_key_wins(k, SgKey{100, 6, 99}));       // then the smaller ext_lo
    CHECK(sg_key_wins(SgKey{100, 7, 8}, k) && !sg_key_wins(k, SgKey{100, 7, 8}));         // then the smaller ext_hi
    CHECK(!sg_key_wins(k, k));
    // the order is total and strict over a small cube
    for (int a = 0; a < 27; ++a)
        for (int b = 0; b < 27; ++b) {
            const SgKey x{a / 9, a / 3 % 3, a % 3}, y{b / 9, b / 3 % 3, b % 3};
            CHECK((a == b) == (!sg_key_wins(x, y) && !sg_key_wins(y, x)));
            CHECK(!(sg_key_wins(x, y) && sg_key_wins(y, x)));
        }
    CHECK(kSgRedFromU == 1 && kSgRedFromW == 2 && kSgUnpaired == 4);
}

static void reducible()
{
    const int32_t M = 2147483647;
    for (int32_t Z : {0, 1, 1000, M}) {
        const int32_t uv = 5000, uw = 9000;
        // the path as long as the arc, then off by Z and by Z + 1, on either side
        CHECK(sg_reducible(uv, uw - uv, uw, Z));
        if (Z < M - uw) {
            CHECK(sg_reducible(uv, uw - uv + Z, uw, Z) && !sg_reducible(uv, uw - uv + Z + 1, uw, Z));
        }
        if (Z < uw - uv - 1) {
            CHECK(sg_reducible(uv, uw - uv - Z, uw, Z) && !sg_reducible(uv, uw - uv - Z - 1, uw, Z));
        }
        // a tie in ext, and the farther arc, never serve as the via -- whatever the fuzz
        CHECK(!sg_reducible(uw, 1, uw, Z) && !sg_reducible(uw + 1, 1, uw, Z) && !sg_reducible(uw, 0, uw, Z));
        CHECK(sg_reducible(uw - 1, 1, uw, Z));
    }
    // the shadowed arc stands: a much shorter path does not remove it
    CHECK(!sg_reducible(1000, 1000, 9000, 1000) && sg_reducible(1000, 7000, 9000, 1000) && !sg_reducible(1000, 6999, 9000, 1000));
    // the sum is taken in 64 bits
    CHECK(!sg_reducible(M - 1, M, M, 1000) && sg_reducible(M - 1, 1, M, 0) && sg_reducible(1, M, M, 1) && !sg_reducible(1, M, M, 0));
    CHECK(sg_reducible(M - 1, M, M, M) && sg_reducible(M - 1, M, M, M - 1) && !sg_reducible(M - 1, M, M, M - 2));
}

int main()
{
    keys();
    const long long n = grid();
    reducible();
    printf("string_graph_rule_check: ok (%lld arcs)\n", n);
    return 0;
}
