// lift_rule_check.cpp -- the rule of include/raft_hip_lift.h as raft_amd/csrc/lift_rule.hpp states it, checked on the CPU as a program
// of its own (tests/test_lift_rule.py builds it under the address and undefined-behaviour sanitizers): fixed cases, the rule's
// properties on random tables with overlapping rows, and spans near 2^31 - 1 on both sides.
#include "../raft_amd/csrc/lift_rule.hpp"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

using namespace raft;

struct Table { std::vector<int64_t> off; std::vector<int32_t> fb, fe; };
struct Rec { int32_t qid, qs, qe, tid, ts, te; bool rev; };
using Out = std::array<int64_t, 7>;                       // qfrag, qs, qe, tfrag, ts, te, rev

static std::vector<Out> lift(const Table &t, const Rec &r, int64_t min_len = 1, int64_t *dropped = nullptr)
{
    std::vector<Out> v;
    lift_record_brute(t.off.data(), t.fb.data(), t.fe.data(), r.qid, r.qs, r.qe, r.tid, r.ts, r.te, r.rev, min_len, dropped,
                      [&](const LiftRecord &o) { v.push_back(Out{o.qfrag, o.qs, o.qe, o.tfrag, o.ts, o.te, r.rev ? 1 : 0}); });
    return v;
}
static Rec mirror(const Rec &r) { return Rec{r.tid, r.ts, r.te, r.qid, r.qs, r.qe, r.rev}; }
static Out mirror(const Out &o) { return Out{o[3], o[4], o[5], o[0], o[1], o[2], o[6]}; }

static Table make_table(const std::vector<std::vector<std::pair<int, int>>> &reads)
{
    Table t;
    t.off.push_back(0);
    for (const auto &rows : reads) {
        for (const auto &row : rows) { t.fb.push_back(row.first); t.fe.push_back(row.second); }
        t.off.push_back((int64_t)t.fb.size());
    }
    return t;
}

// what every output must satisfy: inside its rows and inside the record's sides, spans of at least min_len
static void check_outputs(const Table &t, const Rec &r, const std::vector<Out> &v, int64_t min_len)
{
    for (const Out &o : v) {
        CHECK(o[0] >= t.off[r.qid] && o[0] < t.off[r.qid + 1] && o[3] >= t.off[r.tid] && o[3] < t.off[r.tid + 1]);
        CHECK(0 <= o[1] && o[1] < o[2] && o[2] <= (int64_t)t.fe[o[0]] - t.fb[o[0]]);
        CHECK(0 <= o[4] && o[4] < o[5] && o[5] <= (int64_t)t.fe[o[3]] - t.fb[o[3]]);
        CHECK(o[2] - o[1] >= min_len && o[5] - o[4] >= min_len);
        CHECK(o[1] + t.fb[o[0]] >= r.qs && o[2] + t.fb[o[0]] <= r.qe && o[4] + t.fb[o[3]] >= r.ts && o[5] + t.fb[o[3]] <= r.te);
    }
}

static void check_mirror(const Table &t, const Rec &r, int64_t min_len)
{
    int64_t d0 = 0, d1 = 0;
    std::vector<Out> a = lift(t, r, min_len, &d0), b = lift(t, mirror(r), min_len, &d1);
    check_outputs(t, r, a, min_len);
    check_outputs(t, mirror(r), b, min_len);
    for (Out &o : b) o = mirror(o);
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    CHECK(a == b && d0 == d1);
}

int main()
{
    // -- fixed cases ------------------------------------------------------------------------------------------
    {
        // read 0: one row [0, 1000); read 1: rows [0, 600), [500, 1200); read 2: no rows
        const Table t = make_table({{{0, 1000}}, {{0, 600}, {500, 1200}}, {}});
        // nothing: a read with itself, an empty side, a read without rows, a side beside every row
        CHECK(lift(t, {0, 0, 100, 0, 200, 300, false}).empty());
        CHECK(lift(t, {0, 100, 100, 1, 0, 100, false}).empty() && lift(t, {0, 0, 100, 1, 50, 40, false}).empty());
        CHECK(lift(t, {0, 0, 100, 2, 0, 100, false}).empty() && lift(t, {2, 0, 100, 0, 0, 100, false}).empty());
        CHECK(lift(t, {0, 1000, 1100, 1, 0, 100, false}).empty() && lift(t, {0, 0, 100, 1, 1200, 1300, false}).empty());
        // inside one row on both reads: the record itself, shifted
        std::vector<Out> v = lift(t, {0, 100, 400, 1, 50, 350, false});
        CHECK(v.size() == 1 && v[0] == (Out{0, 100, 400, 1, 50, 350, 0}));
        v = lift(t, {0, 100, 400, 1, 620, 920, true});
        CHECK(v.size() == 1 && v[0] == (Out{0, 100, 400, 2, 120, 420, 1}));
        // the target side [400, 800) meets both rows of read 1, '+', equal spans: [400, 600) of row 1 and [500, 800) of row 2
        v = lift(t, {0, 0, 400, 1, 400, 800, false});
        CHECK(v.size() == 2 && v[0] == (Out{0, 0, 200, 1, 400, 600, 0}) && v[1] == (Out{0, 100, 400, 2, 0, 300, 0}));
        // ... '-': the query's first bases pair with the target's last
        v = lift(t, {0, 0, 400, 1, 400, 800, true});
        CHECK(v.size() == 2 && v[0] == (Out{0, 200, 400, 1, 400, 600, 1}) && v[1] == (Out{0, 0, 300, 2, 0, 300, 1}));
        // ... and the mirror (read 1 is the query: still the B side, its rows are j)
        v = lift(t, {1, 400, 800, 0, 0, 400, false});
        CHECK(v.size() == 2 && v[0] == (Out{1, 400, 600, 0, 0, 200, 0}) && v[1] == (Out{2, 0, 300, 0, 100, 400, 0}));
        // sides that leave the rows are clipped: [-50, 1100) of read 0 against [100, 1250) of read 1 (LA = LB = 1150)
        v = lift(t, {0, -50, 1100, 1, 100, 1250, false});
        CHECK(v.size() == 2 && v[0] == (Out{0, 0, 450, 1, 150, 600, 0}) && v[1] == (Out{0, 350, 1000, 2, 0, 650, 0}));
        // a target twice as long: u = v / 2
        v = lift(t, {0, 100, 300, 1, 400, 800, false});
        CHECK(v.size() == 2 && v[0] == (Out{0, 100, 200, 1, 400, 600, 0}) && v[1] == (Out{0, 150, 300, 2, 0, 300, 0}));
        // min_len: a pair of exactly min_len on the shorter side stays, one base more drops it; the drop is counted
        int64_t dropped = 0;
        v = lift(t, {0, 0, 400, 1, 400, 800, false}, 200, &dropped);
        CHECK(v.size() == 2 && dropped == 0);
        v = lift(t, {0, 0, 400, 1, 400, 800, false}, 201, &dropped);
        CHECK(v.size() == 1 && v[0][3] == 2 && dropped == 1);
        v = lift(t, {0, 0, 400, 1, 400, 800, false}, 301, &dropped);
        CHECK(v.empty() && dropped == 3);
        // step 8 alone: A side long enough, B side one short
        dropped = 0;
        v = lift(t, {0, 0, 400, 1, 0, 100, false}, 101, &dropped);
        CHECK(v.empty() && dropped == 1);
        v = lift(t, {0, 0, 400, 1, 0, 100, false}, 100, &dropped);
        CHECK(v.size() == 1 && v[0] == (Out{0, 0, 400, 1, 0, 100, 0}) && dropped == 1);
        // the pair that leaves neither single row, without a division
        LiftSides s;
        LiftPair p, w;
        CHECK(lift_sides(0, 100, 400, 3, 50, 350, s) && !s.swap && s.LA == 300 && s.LB == 300);
        CHECK(lift_pair_whole(s, 0, 20, 300, w) && lift_pair(s, 0, 1000, 20, 900, false, 300, p));
        CHECK(w.a0 == p.a0 && w.a1 == p.a1 && w.b0 == p.b0 && w.b1 == p.b1 && w.b0 == 30 && w.b1 == 330);
        CHECK(!lift_pair_whole(s, 0, 20, 301, w) && !lift_pair(s, 0, 1000, 20, 900, false, 301, p));
        CHECK(lift_sides(5, 1, 2, 3, 7, 9, s) && s.swap && s.as == 7 && s.ae == 9 && s.bs == 1 && s.be == 2);
        CHECK(!lift_sides(4, 1, 2, 4, 7, 9, s) && !lift_sides(4, 2, 2, 5, 7, 9, s) && !lift_sides(4, 1, 2, 5, 9, 9, s));
    }
    // -- the properties on random tables with overlapping rows ----------------------------------------------------
    {
        std::mt19937_64 rng(12345);
        auto pick = [&](int64_t lo, int64_t hi) { return (int32_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
        const int overlaps[3] = {0, 10, 500};
        for (int round = 0; round < 40; ++round) {
            std::vector<std::vector<std::pair<int, int>>> reads;
            std::vector<int32_t> len;
            const int n_reads = 12;
            for (int r = 0; r < n_reads; ++r) {
                const int k = pick(0, 5);
                std::vector<std::pair<int, int>> rows;
                int pos = pick(0, 40);
                for (int i = 0; i < k; ++i) {
                    const int size = pick(600, 2500);
                    rows.push_back({pos, pos + size});
                    pos += size - overlaps[pick(0, 2)];
                }
                len.push_back((rows.empty() ? 0 : rows.back().second) + pick(1, 400));
                reads.push_back(rows);
            }
            const Table t = make_table(reads);
            for (int k = 0; k < 500; ++k) {
                Rec r;
                r.qid = pick(0, n_reads - 1); r.tid = pick(0, n_reads - 1);
                r.qs = pick(-30, len[r.qid]); r.qe = r.qs + pick(0, len[r.qid] + 30 - r.qs);
                r.ts = pick(-30, len[r.tid]); r.te = r.ts + pick(0, len[r.tid] + 30 - r.ts);
                r.rev = (rng() & 1) != 0;
                const int64_t min_len = (k % 3 == 0) ? 1 : (k % 3 == 1 ? 2 : 501);
                check_mirror(t, r, min_len);
            }
            // one row [0, len) per read: an in-range record lifts to itself
            std::vector<std::vector<std::pair<int, int>>> whole;
            for (int r = 0; r < n_reads; ++r) whole.push_back({{0, len[r]}});
            const Table id = make_table(whole);
            for (int k = 0; k < 500; ++k) {
                Rec r;
                r.qid = pick(0, n_reads - 1); r.tid = pick(0, n_reads - 1);
                r.qs = pick(0, len[r.qid] - 1); r.qe = pick(r.qs + 1, len[r.qid]);
                r.ts = pick(0, len[r.tid] - 1); r.te = pick(r.ts + 1, len[r.tid]);
                r.rev = (rng() & 1) != 0;
                const std::vector<Out> v = lift(id, r);
                if (r.qid == r.tid) { CHECK(v.empty()); continue; }
                CHECK(v.size() == 1 && v[0] == (Out{r.qid, r.qs, r.qe, r.tid, r.ts, r.te, r.rev ? 1 : 0}));
            }
        }
    }
    // -- the 64-bit extremes: spans near 2^31 - 1 on both sides -----------------------------------------------------
    {
        const int32_t M = 2147483647, H = 1 << 30;
        const Table t = make_table({{{0, M}}, {{0, M}}, {{0, H}, {H - 7, M}}, {{0, 3}, {3, M}}});
        std::vector<Out> v = lift(t, {0, 0, M, 1, 0, M, true});
        CHECK(v.size() == 1 && v[0] == (Out{0, 0, M, 1, 0, M, 1}));
        v = lift(t, {1, 0, M, 0, 1, M, false});
        CHECK(v.size() == 1 && v[0] == (Out{1, 0, M, 0, 1, M, 0}));
        for (int rev = 0; rev < 2; ++rev)
            for (int64_t min_len : {(int64_t)1, (int64_t)M - 1, (int64_t)M}) {
                check_mirror(t, {0, 0, M, 2, 0, M, rev != 0}, min_len);
                check_mirror(t, {0, 0, M, 3, 0, M, rev != 0}, min_len);
                check_mirror(t, {2, 0, M, 3, 0, M, rev != 0}, min_len);
                check_mirror(t, {0, M - 2, M, 2, 0, M, rev != 0}, min_len);        // LA = 2 against LB = 2^31 - 1
                check_mirror(t, {0, 0, M, 3, 0, 4, rev != 0}, min_len);            // ... and the other way round
                check_mirror(t, {2, H - 8, H + 1, 3, 2, M, rev != 0}, min_len);
            }
        // both rows of read 2 against the whole of read 0, '+', equal spans: u follows v base by base
        v = lift(t, {0, 0, M, 2, 0, M, false});
        CHECK(v.size() == 2 && v[0] == (Out{0, 0, H, 2, 0, H, 0}) && v[1] == (Out{0, H - 7, M, 3, 0, M - (H - 7), 0}));
    }
    printf("lift_rule_check: ok\n");
    return 0;
}
