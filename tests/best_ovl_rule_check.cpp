// best_ovl_rule_check.cpp -- the rule of include/raft_hip_best.h as raft_amd/csrc/best_ovl_rule.hpp states it, checked on the CPU as a
// program of its own (tests/test_best_ovl_rule.py builds it under the address and undefined-behaviour sanitizers): the key's round
// trips and its order, the partner end, and over a small universe that a set of records counted on both sides gives the table of
// the mirrored set counted on its query sides, in any order of the records, and that mutuality is symmetric.
#include "../raft_amd/csrc/best_ovl_rule.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

using namespace raft;

struct Rec { int q, qs, qe, t, ts, te; bool rev; };

// the table of keys [2 * n_reads] of a set of records, as the public header states it
static std::vector<uint64_t> table(const std::vector<Rec> &recs, const std::vector<int> &len, const std::vector<int> &skip, bool symmetric, int H, int F,
                                   long long *candidates = nullptr, long long *left_out = nullptr)
{
    std::vector<uint64_t> tab(2 * len.size(), 0);
    long long cand = 0, left = 0;
    for (const Rec &r : recs) {
        const int kind = ends_kind(r.q, r.qs, r.qe, len[(size_t)r.q], r.t, r.ts, r.te, len[(size_t)r.t], r.rev, H, F);
        const int span = std::min(r.qe - r.qs, r.te - r.ts);
        const int view[2] = {kind, ends_target_view(kind, r.rev)}, me[2] = {r.q, r.t}, other[2] = {r.t, r.q};
        for (int v = 0; v < (symmetric ? 1 : 2); ++v) {
            const int e = best_end_of(view[v]);
            if (e < 0) continue;
            if (skip[(size_t)r.q] || skip[(size_t)r.t]) { ++left; continue; }
            ++cand;
            uint64_t &slot = tab[2 * (size_t)me[v] + (size_t)e];
            slot = std::max(slot, best_pack(span, other[v], r.rev));
        }
    }
    if (candidates) *candidates = cand;
    if (left_out) *left_out = left;
    return tab;
}

static std::vector<Rec> with_mirrors(const std::vector<Rec> &recs)
{
    std::vector<Rec> all(recs);
    for (const Rec &r : recs) all.push_back(Rec{r.t, r.ts, r.te, r.q, r.qs, r.qe, r.rev});
    return all;
}

// every mutual slot's partner slot is mutual and points back; -> the number of mutual slots
static long long check_mutual(const std::vector<uint64_t> &tab)
{
    long long mutual = 0;
    const int n = (int)tab.size() / 2;
    for (int r = 0; r < n; ++r)
        for (int e = 0; e < 2; ++e) {
            const uint64_t mine = tab[2 * (size_t)r + (size_t)e];
            if (!mine) continue;
            const int p = best_partner(mine), pe = best_partner_end(e, best_rev(mine));
            CHECK(p >= 0 && p < n && p != r);
            const uint64_t theirs = tab[2 * (size_t)p + (size_t)pe];
            if (!best_mutual(r, e, mine, theirs)) continue;
            ++mutual;
            CHECK(best_mutual(p, pe, theirs, mine));
            CHECK(best_partner(theirs) == r && best_partner_end(pe, best_rev(theirs)) == e);
            CHECK(best_span(theirs) == best_span(mine) && best_rev(theirs) == best_rev(mine));   // (both chose the same overlap, or its equal)
        }
    CHECK(mutual % 2 == 0);
    return mutual;
}

static void keys()
{
    const int32_t M = 2147483647;
    for (int32_t span : {1, 2, 1000, M})
        for (int32_t other : {0, 1, 77, M - 1})
            for (int rev = 0; rev < 2; ++rev) {
                const uint64_t k = best_pack(span, other, rev != 0);
                CHECK(k != 0 && best_span(k) == span && best_partner(k) == other && best_rev(k) == (rev != 0));
                CHECK((k & 1) == 0);
            }
    CHECK(best_pack(1, M - 1, false) == ((1ull << 33) | 4));   // the smallest key of all: the largest id a set of 2^31 - 1 reads has
    CHECK(best_pack(M, 0, true) == (((uint64_t)M << 33) | (0x7FFFFFFFull << 2) | 2));
    // the order: span decides, then the smaller partner, then '-' before '+'
    CHECK(best_pack(2, M - 1, false) > best_pack(1, 0, true));
    CHECK(best_pack(1000, 5, false) > best_pack(999, 0, true) && best_pack(M, 7, false) > best_pack(M - 1, 7, true));
    CHECK(best_pack(1000, 4, false) > best_pack(1000, 5, true) && best_pack(1000, 0, false) > best_pack(1000, M - 1, true));
    CHECK(best_pack(1000, 5, true) > best_pack(1000, 5, false));
    CHECK(best_pack(1000, 5, true) == best_pack(1000, 5, true));
    // the partner's end: the other end on '+', the same end on '-'
    CHECK(best_partner_end(0, false) == 1 && best_partner_end(1, false) == 0 && best_partner_end(0, true) == 0 && best_partner_end(1, true) == 1);
    CHECK(best_end_of(kEndQuery5) == 0 && best_end_of(kEndQuery3) == 1);
    for (int k : {kEndInvalid, kEndInternal, kEndQueryContained, kEndTargetContained, kEndSelf, 7, -1}) CHECK(best_end_of(k) == -1);
    CHECK(!best_mutual(0, 0, 0, best_pack(5, 0, false)) && !best_mutual(0, 0, best_pack(5, 1, false), 0));
    CHECK(best_mutual(0, 1, best_pack(5, 1, false), best_pack(5, 0, false)) && !best_mutual(0, 1, best_pack(5, 1, false), best_pack(5, 2, false)));
    CHECK(kBestRev5 == 1 && kBestMutual5 == 2 && kBestRev3 == 4 && kBestMutual3 == 8 && kBestSkipped == 16);
}

// Reads 0, 1 and 2 of lengths l0, l1 and l1: every valid record of 0 against 1, of 1 against 0 and of 2 against 0, on both strands.
// One record at a time and all of them together, as given and in reverse order, with and without read 2 left out.
static long long universe()
{
    long long n = 0, slots = 0, mutual = 0, left = 0;
    for (int l0 = 1; l0 <= 5; ++l0)
        for (int l1 = 1; l1 <= 5; ++l1)
            for (int H : {0, 1})
                for (int F : {0, 800}) {
                    const std::vector<int> len = {l0, l1, l1};
                    const int pairs[][2] = {{0, 1}, {1, 0}, {2, 0}};
                    std::vector<Rec> all;
                    for (const auto &p : pairs)
                        for (int qs = 0; qs < len[(size_t)p[0]]; ++qs)
                            for (int qe = qs + 1; qe <= len[(size_t)p[0]]; ++qe)
                                for (int ts = 0; ts < len[(size_t)p[1]]; ++ts)
                                    for (int te = ts + 1; te <= len[(size_t)p[1]]; ++te)
                                        for (int rev = 0; rev < 2; ++rev) all.push_back(Rec{p[0], qs, qe, p[1], ts, te, rev != 0});
                    const std::vector<int> nobody = {0, 0, 0}, two = {0, 0, 1};
                    for (const Rec &r : all) {
                        const std::vector<Rec> one = {r};
                        const std::vector<uint64_t> both = table(one, len, nobody, false, H, F);
                        CHECK(both == table(with_mirrors(one), len, nobody, true, H, F));
                        check_mutual(both);
                        ++n;
                    }
                    for (const std::vector<int> &skip : {nobody, two}) {
                        long long c2 = 0, o2 = 0, c1 = 0, o1 = 0;
                        const std::vector<uint64_t> both = table(all, len, skip, false, H, F, &c2, &o2);
                        std::vector<Rec> full = with_mirrors(all);
                        CHECK(both == table(full, len, skip, true, H, F, &c1, &o1));
                        CHECK(c1 == c2 && o1 == o2);                   // (counted in views)
                        std::reverse(full.begin(), full.end());
                        CHECK(both == table(full, len, skip, true, H, F));
                        std::vector<Rec> back(all.rbegin(), all.rend());
                        CHECK(both == table(back, len, skip, false, H, F));
                        mutual += check_mutual(both);
                        for (uint64_t k : both) slots += k != 0;
                        if (skip[2]) { CHECK(both[4] == 0 && both[5] == 0); left += o2; }
                        for (size_t s = 0; s < 4; ++s) CHECK(!skip[2] || both[s] == 0 || best_partner(both[s]) != 2);
                    }
                }
    CHECK(slots > 0 && mutual > 0 && left > 0);            // (the universe holds what it is about)
    return n;
}

int main()
{
    keys();
    const long long n = universe();
    printf("best_ovl_rule_check: ok (%lld records)\n", n);
    return 0;
}
