// unitig_rule_check.cpp -- the rule of include/raft_hip_utg.h as raft_amd/csrc/unitig_rule.hpp states it, checked on the CPU as a program
// of its own (tests/test_unitig_rule.py builds it under the address and undefined-behaviour sanitizers): twin, succ and w on hand-made
// tables, the consistency rule on one table per violated condition, and a sequential walk -- written here, over succ alone -- on a '+'
// chain, a mixed-strand chain, the 2-cycle in both strand forms and a 3-cycle.
#include "../raft_amd/csrc/unitig_rule.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

using namespace raft;

struct Table {
    std::vector<int32_t> len, partner, span;
    std::vector<uint8_t> flags;
    explicit Table(std::vector<int32_t> l) : len(std::move(l)), partner(2 * len.size(), -1), span(2 * len.size(), 0), flags(len.size(), 0) {}
    int32_t n() const { return (int32_t)len.size(); }
    // a mutual overlap of s bases between end ea of a and end eb of b (the strand follows from the ends: '-' iff they are the same end)
    void link(int32_t a, int ea, int32_t b, int eb, int32_t s)
    {
        const unsigned rev = ea == eb ? (unsigned)kBestRev5 : 0u;
        partner[2 * a + ea] = b; span[2 * a + ea] = s; flags[a] |= (uint8_t)((kBestMutual5 | rev) << (2 * ea));
        partner[2 * b + eb] = a; span[2 * b + eb] = s; flags[b] |= (uint8_t)((kBestMutual5 | rev) << (2 * eb));
    }
    bool ok(int32_t r, int e) const { return utg_end_ok(n(), len.data(), partner.data(), span.data(), flags.data(), r, e); }
    int32_t first_bad() const
    {
        for (int32_t r = 0; r < n(); ++r)
            if (!ok(r, 0) || !ok(r, 1)) return r;
        return -1;
    }
    int32_t succ(int32_t h) const { return utg_succ(partner.data(), flags.data(), utg_read(h), utg_end(h)); }
    int64_t w(int32_t h) const { return utg_weight(len.data(), partner.data(), span.data(), utg_read(h), utg_end(h)); }
};

struct Layout {
    std::vector<int32_t> unitig, index, order, utg_reads;
    std::vector<int64_t> offset, utg_off, utg_length;
    std::vector<uint8_t> orient, utg_circular;
};

// the walk of the header, one read after the other, over succ and w alone
Layout walk(const Table &t)
{
    const int32_t n = t.n();
    struct Start { int32_t read; int32_t half; bool circular; };
    std::vector<Start> starts;
    std::vector<char> seen((size_t)n, 0);
    for (int32_t r = 0; r < n; ++r) {
        if (utg_skipped(t.flags[r]) || seen[r]) continue;
        seen[r] = 1;
        int32_t term[2];
        bool circular = false;
        for (int e = 0; e < 2 && !circular; ++e) {
            int32_t h = utg_half(r, e);
            while (t.succ(h) != kUtgNil) {
                h = t.succ(h);
                if (utg_read(h) == r) { circular = true; break; }
                seen[utg_read(h)] = 1;
            }
            term[e] = h;                                   // the half-edge through the terminal's free end
        }
        if (circular) starts.push_back({r, utg_half(r, 1), true});         // (r is the smallest read of its cycle: all before it are seen)
        else if (utg_read(term[0]) == utg_read(term[1])) starts.push_back({r, utg_half(r, 1), false});
        else {
            const int32_t free_half = utg_read(term[0]) < utg_read(term[1]) ? term[0] : term[1];
            starts.push_back({utg_read(free_half), utg_twin(free_half), false});
        }
    }
    std::sort(starts.begin(), starts.end(), [](const Start &a, const Start &b) { return a.read < b.read; });
    Layout o;
    o.unitig.assign((size_t)n, -1); o.index.assign((size_t)n, -1); o.offset.assign((size_t)n, 0); o.orient.assign((size_t)n, 0);
    o.utg_off.push_back(0);
    for (size_t u = 0; u < starts.size(); ++u) {
        int32_t h = starts[u].half, k = 0;
        int64_t off = 0, length = 0;
        for (;;) {
            const int32_t r = utg_read(h);
            o.unitig[r] = (int32_t)u; o.index[r] = k++; o.offset[r] = off; o.orient[r] = (uint8_t)(1 - utg_end(h));
            o.order.push_back(r);
            const int32_t nx = t.succ(h);
            if (nx == kUtgNil) { length = off + utg_len(t.len[r]); break; }
            off += t.w(h) - utg_len(t.len[utg_read(nx)]) + utg_len(t.len[r]);      // len(r) - span(r -> next)
            if (starts[u].circular && utg_read(nx) == starts[u].read) { length = off; break; }
            h = nx;
        }
        o.utg_off.push_back((int64_t)o.order.size()); o.utg_reads.push_back(k); o.utg_length.push_back(length);
        o.utg_circular.push_back(starts[u].circular ? 1 : 0);
    }
    return o;
}

template <class T> bool same(const std::vector<T> &a, std::initializer_list<long long> b)
{
    if (a.size() != b.size()) return false;
    size_t i = 0;
    for (long long x : b)
        if ((long long)a[i++] != x) return false;
    return true;
}

int main()
{
    // ---- half-edges
    CHECK(utg_half(7, 1) == 15 && utg_read(15) == 7 && utg_end(15) == 1 && utg_end(14) == 0 && utg_twin(15) == 14 && utg_twin(14) == 15);
    CHECK(utg_twin(0) == 1 && utg_twin(utg_twin(2147483645)) == 2147483645 && utg_half(kUtgMaxReads - 1, 1) == 2147483645);
    CHECK(utg_len(-1) == 0 && utg_len(-2147483647 - 1) == 0 && utg_len(0) == 0 && utg_len(2147483647) == 2147483647);
    CHECK(utg_rounds(0) == 0 && utg_rounds(1) == 1 && utg_rounds(2) == 2 && utg_rounds(3) == 3 && utg_rounds(4) == 3 && utg_rounds(5) == 4);
    CHECK(utg_rounds(1024) == 11 && utg_rounds(1025) == 12 && utg_rounds(kUtgMaxReads) == 31);

    // ---- succ and w: a3 - b5 on '+' (100 bases), b3 - c3 on '-' (30 bases)
    {
        Table t({1000, 2000, 500, 700});
        t.link(0, 1, 1, 0, 100);
        t.link(1, 1, 2, 1, 30);
        CHECK(t.first_bad() == -1);
        CHECK(t.flags[0] == kBestMutual3 && t.flags[1] == (kBestMutual5 | kBestMutual3 | kBestRev3) && t.flags[2] == (kBestMutual3 | kBestRev3));
        CHECK(t.succ(utg_half(0, 1)) == utg_half(1, 1) && t.w(utg_half(0, 1)) == 2000 - 100);      // enters b at 5', leaves through 3'
        CHECK(t.succ(utg_half(1, 1)) == utg_half(2, 0) && t.w(utg_half(1, 1)) == 500 - 30);        // enters c at 3', leaves through 5'
        CHECK(t.succ(utg_half(2, 0)) == kUtgNil && t.succ(utg_half(0, 0)) == kUtgNil && t.succ(utg_half(3, 0)) == kUtgNil && t.succ(utg_half(3, 1)) == kUtgNil);
        // the mirror: succ(twin(succ(h))) == twin(h)
        CHECK(t.succ(utg_half(2, 1)) == utg_half(1, 0) && t.w(utg_half(2, 1)) == 2000 - 30);
        CHECK(t.succ(utg_half(1, 0)) == utg_half(0, 0) && t.w(utg_half(1, 0)) == 1000 - 100);
        for (int32_t h = 0; h < 8; ++h)
            if (t.succ(h) != kUtgNil) CHECK(t.succ(utg_twin(t.succ(h))) == utg_twin(h));
        // a length below 0 counts as 0 in w
        t.len[1] = -5;
        CHECK(t.w(utg_half(0, 1)) == -100);
    }

    // ---- the consistency rule: one table per violated condition, from a sound one (reads 0 - 1 - 2, read 3 skipped, read 4 alone)
    {
        const auto sound = [] {
            Table t({1000, 2000, 500, 700, 900});
            t.link(0, 1, 1, 0, 100);
            t.link(1, 1, 2, 1, 30);
            t.flags[3] = kBestSkipped;
            return t;
        };
        CHECK(sound().first_bad() == -1);
        // what is not mutual is not looked at
        { Table t = sound(); t.partner[2 * 4] = 99; t.span[2 * 4] = -7; t.flags[4] = kBestRev5 | kBestRev3; t.partner[0] = -9; CHECK(t.first_bad() == -1); }
        { Table t = sound(); t.partner[2 * 3 + 1] = 3; t.flags[3] |= kBestRev3; CHECK(t.first_bad() == -1); }
        { Table t = sound(); t.flags[1] |= kBestSkipped; CHECK(!t.ok(1, 0) && !t.ok(1, 1) && !t.ok(0, 1) && !t.ok(2, 1) && t.first_bad() == 0); }     // r SKIPPED (and p, seen from 0)
        { Table t = sound(); t.partner[2 * 1 + 1] = -1; CHECK(t.ok(1, 0) && !t.ok(1, 1) && t.first_bad() == 1); }                    // p below 0
        { Table t = sound(); t.partner[2 * 1 + 1] = 5; CHECK(!t.ok(1, 1) && t.first_bad() == 1); }                                  // p == n_reads
        { Table t = sound(); t.partner[2 * 1 + 1] = 2147483647; CHECK(!t.ok(1, 1)); }
        { Table t = sound(); t.partner[2 * 1 + 1] = 1; CHECK(!t.ok(1, 1) && t.first_bad() == 1); }                                  // p == r
        { Table t = sound(); t.partner[2 * 1 + 1] = 3; CHECK(!t.ok(1, 1) && t.first_bad() == 1); }                                  // p SKIPPED
        { Table t = sound(); t.flags[2] &= (uint8_t)~kBestMutual3; CHECK(!t.ok(1, 1) && t.ok(2, 1) && t.first_bad() == 1); }        // no MUTUAL at E'
        { Table t = sound(); t.flags[2] &= (uint8_t)~kBestRev3; CHECK(!t.ok(1, 1) && !t.ok(2, 1) && t.first_bad() == 1); }          // the REV bits differ
        { Table t = sound(); t.partner[2 * 2 + 1] = 0; CHECK(!t.ok(1, 1) && !t.ok(2, 1) && t.first_bad() == 1); }                   // does not lead back
        { Table t = sound(); t.span[2 * 2 + 1] = 31; CHECK(!t.ok(1, 1) && !t.ok(2, 1) && t.ok(1, 0) && t.first_bad() == 1); }       // the spans differ
        { Table t = sound(); t.span[2 * 1 + 1] = t.span[2 * 2 + 1] = 0; CHECK(!t.ok(1, 1) && !t.ok(2, 1)); }                        // span below 1
        { Table t = sound(); t.span[2 * 1 + 1] = t.span[2 * 2 + 1] = 500; CHECK(t.first_bad() == -1); }                             // span == the shorter length
        { Table t = sound(); t.span[2 * 1 + 1] = t.span[2 * 2 + 1] = 501; CHECK(!t.ok(1, 1) && !t.ok(2, 1) && t.first_bad() == 1); }
        { Table t = sound(); t.len[2] = -1; CHECK(!t.ok(1, 1) && !t.ok(2, 1) && t.ok(0, 1)); }                                      // a length below 0 counts as 0
    }

    // ---- the walk
    {   // a '+' chain 3 -> 0 -> 2 (read 1 alone, read 4 skipped): the terminal with the smaller id, 2, is the start, so everybody is '-'
        Table t({1000, 400, 600, 800, 50});
        t.link(3, 1, 0, 0, 100);
        t.link(0, 1, 2, 0, 200);
        t.flags[4] = kBestSkipped;
        CHECK(t.first_bad() == -1);
        const Layout o = walk(t);
        CHECK(same(o.unitig, {1, 0, 1, 1, -1}) && same(o.index, {1, 0, 0, 2, -1}) && same(o.orient, {1, 0, 1, 1, 0}));
        CHECK(same(o.offset, {400, 0, 0, 1300, 0}) && same(o.order, {1, 2, 0, 3}) && same(o.utg_off, {0, 1, 4}));
        CHECK(same(o.utg_reads, {1, 3}) && same(o.utg_length, {400, 2100}) && same(o.utg_circular, {0, 0}));
    }
    {   // a mixed-strand chain: 0(3') - 1(3') on '-', 1(5') - 2(5') on '-', 2(3') - 3(5') on '+'
        Table t({1000, 2000, 3000, 4000});
        t.link(0, 1, 1, 1, 10);
        t.link(1, 0, 2, 0, 20);
        t.link(2, 1, 3, 0, 30);
        CHECK(t.first_bad() == -1);
        const Layout o = walk(t);
        CHECK(same(o.unitig, {0, 0, 0, 0}) && same(o.index, {0, 1, 2, 3}) && same(o.orient, {0, 1, 0, 0}));
        CHECK(same(o.offset, {0, 990, 2970, 5940}) && same(o.order, {0, 1, 2, 3}) && same(o.utg_length, {9940}) && same(o.utg_circular, {0}));
    }
    {   // the 2-cycle on '+': a3 - b5, b3 - a5 (a = 2, b = 1: the start is 1)
        Table t({70, 1000, 3000});
        t.link(2, 1, 1, 0, 100);
        t.link(1, 1, 2, 0, 200);
        CHECK(t.first_bad() == -1);
        CHECK(t.succ(utg_half(1, 1)) == utg_half(2, 1) && t.succ(utg_half(2, 1)) == utg_half(1, 1));
        CHECK(t.succ(utg_half(1, 0)) == utg_half(2, 0) && t.succ(utg_half(2, 0)) == utg_half(1, 0));
        const Layout o = walk(t);
        CHECK(same(o.unitig, {0, 1, 1}) && same(o.index, {0, 0, 1}) && same(o.orient, {0, 0, 0}) && same(o.offset, {0, 0, 800}));
        CHECK(same(o.order, {0, 1, 2}) && same(o.utg_reads, {1, 2}) && same(o.utg_length, {70, 800 + 2900}) && same(o.utg_circular, {0, 1}));
    }
    {   // the 2-cycle on '-': a3 - b3, a5 - b5
        Table t({1000, 3000});
        t.link(0, 1, 1, 1, 100);
        t.link(0, 0, 1, 0, 200);
        CHECK(t.first_bad() == -1);
        CHECK(t.succ(utg_half(0, 1)) == utg_half(1, 0) && t.succ(utg_half(1, 0)) == utg_half(0, 1));
        CHECK(t.succ(utg_half(0, 0)) == utg_half(1, 1) && t.succ(utg_half(1, 1)) == utg_half(0, 0));
        const Layout o = walk(t);
        CHECK(same(o.unitig, {0, 0}) && same(o.index, {0, 1}) && same(o.orient, {0, 1}) && same(o.offset, {0, 900}));
        CHECK(same(o.order, {0, 1}) && same(o.utg_reads, {2}) && same(o.utg_length, {900 + 2800}) && same(o.utg_circular, {1}));
    }
    {   // a 3-cycle 1 -> 3 -> 2 -> 1 with one '-' pair of edges (read 3 is reversed), read 0 alone with a length below 0
        Table t({-4, 1000, 2000, 3000});
        t.link(1, 1, 3, 1, 10);          // leaves 1 through 3', enters 3 at its 3'
        t.link(3, 0, 2, 0, 20);          // leaves 3 through 5', enters 2 at its 5'
        t.link(2, 1, 1, 0, 30);          // leaves 2 through 3', enters 1 at its 5'
        CHECK(t.first_bad() == -1);
        const Layout o = walk(t);
        CHECK(same(o.unitig, {0, 1, 1, 1}) && same(o.index, {0, 0, 2, 1}) && same(o.orient, {0, 0, 0, 1}));
        CHECK(same(o.offset, {0, 0, 990 + 2980, 990}) && same(o.order, {0, 1, 3, 2}) && same(o.utg_off, {0, 1, 4}));
        CHECK(same(o.utg_reads, {1, 3}) && same(o.utg_length, {0, 990 + 2980 + 1970}) && same(o.utg_circular, {0, 1}));
        // every half-edge of the cycle comes back to itself after three steps, and never meets its twin
        for (int32_t h = 2; h < 8; ++h) {
            CHECK(t.succ(t.succ(t.succ(h))) == h);
            CHECK(t.succ(h) != utg_twin(h) && t.succ(t.succ(h)) != utg_twin(h));
        }
    }
    {   // no reads
        const Layout o = walk(Table({}));
        CHECK(o.order.empty() && same(o.utg_off, {0}) && o.utg_reads.empty());
    }
    printf("unitig_rule_check: ok\n");
    return 0;
}
