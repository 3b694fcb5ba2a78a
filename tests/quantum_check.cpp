// quantum_check.cpp -- raft_amd/csrc/quantum.hpp on the CPU (tests/test_quantum.py builds it with the host compiler under the address
// and undefined-behaviour sanitizers and runs it as a process of its own).
//
//   quantum_check                 every check below over the list of window counts; prints "quantum_check: ok"
//   quantum_check print <B>       "graded <B> share <share> n_long <n_long> per_share <per_share>" and one line "<k> <at(k)>" per boundary
//   quantum_check print <B> <q>   the same for the uniform quantum q: "uniform <B> q <q> n_ranges <n>"
//
// The boundaries are defined FORWARDS here, from the comment above Quantum and not from idx(): share s begins at s * share, its
// first n_long ranges are q_long long, the ranges behind them q_short.  share, n_long and per_share are worked out again in integers.
#include "../raft_amd/csrc/quantum.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using raft::Quantum;

namespace {

constexpr int kQLong = 31744, kQShort = 7936;       // eight and two tiles' worth (engine.hip quantum_for)
constexpr long long kTwo31 = 1LL << 31;
int failures = 0;

#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++failures <= 20) { printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                       \
    } while (0)

struct Graded {                 // the geometry, worked out here
    long long B, share;
    long long n_long, per_share;
    long long at(long long k) const
    {
        const long long s = k / per_share, j = k % per_share;
        if (k >= 8 * per_share) return 8 * share;
        return s * share + (j <= n_long ? j * kQLong : n_long * kQLong + (j - n_long) * kQShort);
    }
};

Graded graded_geometry(long long B)
{
    Graded g{};
    g.B = B;
    long long eighth = B / 8 + (B % 8 ? 1 : 0);
    g.share = eighth;
    while (g.share % 128) ++g.share;
    g.n_long = g.share * 9 / (10LL * kQLong);                  // nine tenths of a share, whole long ranges
    const long long rest = g.share - g.n_long * kQLong;
    g.per_share = g.n_long + rest / kQShort + (rest % kQShort ? 1 : 0);
    return g;
}

// idx against at() next to every boundary, and over a sweep of windows
void check_graded(long long B, bool full_sweep)
{
    const Graded g = graded_geometry(B);
    const Quantum z = raft::graded_quantum(B, kQLong, kQShort, 0.9);
    CHECK(z.share == g.share && z.n_long == g.n_long && z.per_share == g.per_share && z.q_long == kQLong && z.q_short == kQShort,
          "B %lld: graded_quantum gives share %lld n_long %d per_share %d, the integers give %lld %lld %lld", B, z.share, z.n_long, z.per_share,
          g.share, g.n_long, g.per_share);
    if (z.share != g.share || z.n_long != g.n_long || z.per_share != g.per_share) return;
    CHECK(g.share % 128 == 0 && g.share * 8 >= B && (g.share - 128) * 8 < B && g.share < kTwo31, "B %lld share %lld", B, g.share);
    CHECK(g.per_share >= 1, "B %lld per_share %lld", B, g.per_share);
    CHECK(z.n_ranges(B) == 8 * g.per_share, "B %lld n_ranges %lld per_share %lld", B, z.n_ranges(B), g.per_share);
    // the long part lies inside the share; the share's last range is no longer than q_short and longer than 0: the clamp of idx()
    // (j < per_share) then never takes effect for x < share, because the unclamped j reaches per_share only at
    // x >= n_long * q_long + (per_share - n_long) * q_short >= share
    const long long last = g.share - (g.at(g.per_share - 1) - g.at(0));
    CHECK(g.n_long * kQLong <= g.share, "B %lld: the long ranges leave the share", B);
    CHECK(last > 0 && last <= kQShort, "B %lld: a share's last range is %lld windows", B, last);
    CHECK(g.n_long * kQLong + (g.per_share - g.n_long) * kQShort >= g.share, "B %lld: the clamp of idx() takes effect inside a share", B);
    const long long n = 8 * g.per_share;
    for (long long s = 0; s <= 8; ++s) CHECK(g.at(s * g.per_share) == s * g.share, "B %lld share %lld begins at %lld", B, s, g.at(s * g.per_share));
    for (long long k = 0; k <= n; ++k) {
        const long long a = g.at(k);
        if (k < n) CHECK(g.at(k + 1) > a, "B %lld k %lld: at does not ascend (%lld, %lld)", B, k, a, g.at(k + 1));
        CHECK(z.idx(a) == k, "B %lld k %lld: idx(at(k) = %lld) = %lld", B, k, a, z.idx(a));
        if (k > 0) CHECK(z.idx(a - 1) == k - 1, "B %lld k %lld: idx(at(k) - 1 = %lld) = %lld", B, k, a - 1, z.idx(a - 1));
        if (k == n || a + 1 < g.at(k + 1)) CHECK(z.idx(a + 1) == k, "B %lld k %lld: idx(at(k) + 1 = %lld) = %lld", B, k, a + 1, z.idx(a + 1));
    }
    // behind every share: the closing boundary
    for (long long w : {8 * g.share, 8 * g.share + 1, 8 * g.share + kQShort, 8 * g.share + kQLong + 1, 16 * g.share, 8 * g.share + kTwo31, 1LL << 40})
        CHECK(z.idx(w) == n, "B %lld: idx(%lld) = %lld behind every share, want %lld", B, w, z.idx(w), n);
    // idx never descends, and steps by one exactly on the boundaries: every window (small sets), or a stride with every boundary's surroundings
    const long long end = 8 * g.share + 2 * kQLong;
    const long long stride = full_sweep ? 1 : 997;
    long long prev = 0, k_next = 1;
    for (long long w = 0; w < end; w += stride) {
        const long long i = z.idx(w);
        CHECK(i >= prev, "B %lld: idx descends at window %lld (%lld after %lld)", B, w, i, prev);
        if (full_sweep) {
            while (k_next <= n && g.at(k_next) <= w) ++k_next;
            CHECK(i == k_next - 1, "B %lld: idx(%lld) = %lld, the largest k with at(k) <= w is %lld", B, w, i, k_next - 1);
        } else {
            CHECK(i <= n && g.at(i) <= w && (i == n || g.at(i + 1) > w), "B %lld: idx(%lld) = %lld is not the largest k with at(k) <= w", B, w, i);
        }
        prev = i;
        if (failures > 20) return;
    }
}

void check_uniform(int q)
{
    const Quantum z = raft::uniform_quantum(q);
    CHECK(z.share == 0 && z.q == q, "uniform_quantum(%d)", q);
    // around 0, around 2^31 (idx divides in 32 bits below it) and far behind it
    const long long centres[] = {0, 1000LL * q, kTwo31 / q * q, (kTwo31 / q + 1) * q, 3 * kTwo31 / q * q, (1LL << 40) / q * q};
    for (long long c : centres)
        for (long long k = c / q - (c ? 3 : 0); k <= c / q + 3; ++k) {
            const long long a = k * q;
            CHECK(z.idx(a) == k, "q %d k %lld: idx(%lld) = %lld", q, k, a, z.idx(a));
            if (k > 0) CHECK(z.idx(a - 1) == k - 1, "q %d k %lld: idx(%lld) = %lld", q, k, a - 1, z.idx(a - 1));
            CHECK(z.idx(a + 1) == k, "q %d k %lld: idx(%lld) = %lld", q, k, a + 1, z.idx(a + 1));
        }
    long long prev = 0;
    for (long long w = 0; w < 40LL * q; ++w) {
        const long long i = z.idx(w);
        CHECK(i >= prev && i == w / q, "q %d: idx(%lld) = %lld", q, w, i);
        prev = i;
    }
    for (long long w = kTwo31 - 2LL * q; w < kTwo31 + 2LL * q; ++w) {
        const long long i = z.idx(w);
        CHECK(i >= prev && i == w / q, "q %d: idx(%lld) = %lld", q, w, i);
        prev = i;
    }
    for (long long B : {0LL, 1LL, (long long)q - 1, (long long)q, (long long)q + 1, 1000000LL, kTwo31 - 1, kTwo31, kTwo31 + q})
        CHECK(z.n_ranges(B) == B / q + 1 && z.idx(B) + 1 == z.n_ranges(B), "q %d B %lld: n_ranges %lld", q, B, z.n_ranges(B));
}

int print_mode(int argc, char **argv)
{
    const long long B = atoll(argv[2]);
    if (argc > 3) {
        const int q = atoi(argv[3]);
        const Quantum z = raft::uniform_quantum(q);
        const long long n = z.n_ranges(B);
        printf("uniform %lld q %d n_ranges %lld\n", B, q, n);
        for (long long k = 0; k <= n; ++k) {
            if (z.idx(k * q) != k) { printf("idx(%lld) = %lld, want %lld\n", k * q, z.idx(k * q), k); return 1; }
            printf("%lld %lld\n", k, k * q);
        }
        return 0;
    }
    const Graded g = graded_geometry(B);
    const Quantum z = raft::graded_quantum(B, kQLong, kQShort, 0.9);
    if (z.share != g.share || z.n_long != g.n_long || z.per_share != g.per_share) { printf("graded_quantum(%lld) and the integers disagree\n", B); return 1; }
    printf("graded %lld share %lld n_long %lld per_share %lld\n", B, g.share, g.n_long, g.per_share);
    for (long long k = 0; k <= 8 * g.per_share; ++k) {
        if (z.idx(g.at(k)) != k) { printf("idx(%lld) = %lld, want %lld\n", g.at(k), z.idx(g.at(k)), k); return 1; }
        printf("%lld %lld\n", k, g.at(k));
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "print")) return print_mode(argc, argv);
    for (int q : {256, 7936, 11904}) check_uniform(q);
    // the largest set quantum_for still grades ((B + 7) / 8 + 128 < 2^31), and the first it does not
    const long long b_max = 8 * (kTwo31 - 129);
    CHECK((b_max + 7) / 8 + 128 < kTwo31 && !((b_max + 1 + 7) / 8 + 128 < kTwo31), "the largest graded set is not %lld", b_max);
    const long long small[] = {1, 100, 128, 129, 1024, 1025, 8 * 7936, 8 * 7936 + 1, 200000, 281600, 281601, 888831, 888832, 888833, 1000000,
                               2539520 /* nine tenths of a share is nine long ranges exactly */, 5840000, 5840896, 5840897 /* 256 boundaries, and the first set with more */, 5900000};
    for (long long B : small) check_graded(B, true);
    for (long long B : {1072693248LL, b_max, b_max + 1}) check_graded(B, false);
    // what the list is there for
    CHECK(graded_geometry(100).share == 128 && graded_geometry(100).per_share == 1, "B 100");
    CHECK(graded_geometry(281600).n_long == 0 && graded_geometry(281601).n_long == 1, "n_long 0 -> 1");
    CHECK((graded_geometry(888832).share - graded_geometry(888832).n_long * kQLong) % kQShort == 0, "888832: no short closing range");
    CHECK((graded_geometry(888833).share - graded_geometry(888833).n_long * kQLong) % kQShort == 128, "888833: a closing range of 128 windows");
    CHECK(8 * graded_geometry(5840896).per_share == 256 && 8 * graded_geometry(5840897).per_share > 256, "more than 256 boundaries from 5,840,897 windows on");
    if (failures) { printf("quantum_check: %d check(s) failed\n", failures); return 1; }
    printf("quantum_check: ok\n");
    return 0;
}
