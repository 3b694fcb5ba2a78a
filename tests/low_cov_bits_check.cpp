// low_cov_bits_check.cpp -- the word arithmetic of raft_amd/csrc/low_cov_bits.hpp against a loop that looks at one window at a time:
// start bits, end bits and the open-at-the-left-edge bit of every word, the ranks the kernels derive from them (the k-th start and
// the k-th end of the array are one run's; a word whose first window continues a run ranks its ends one lower), the valid mask of
// the array's last, partial word, the class bits and the uncovered bit.  Built by the host compiler alone, under the sanitizers
// (tests/test_low_cov_bits.py).
#include "../raft_amd/csrc/low_cov_bits.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace raft;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (++failures < 20) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                   \
    } while (0)

struct Run { long long first, last; };

// the definition: windows 0..n-1, low[w], rs[w] (w begins a read); runs never continue across a read's first window
std::vector<Run> runs_by_loop(const std::vector<int> &low, const std::vector<int> &rs)
{
    std::vector<Run> out;
    const long long n = (long long)low.size();
    long long w = 0;
    while (w < n) {
        if (!low[(size_t)w]) { ++w; continue; }
        const long long a = w;
        ++w;
        while (w < n && low[(size_t)w] && !rs[(size_t)w]) ++w;
        out.push_back({a, w - 1});
    }
    return out;
}

// the kernels' way: per word starts / ends / open, ranked by popcount prefixes over the words
void check_array(const std::vector<int> &low, const std::vector<int> &rs, const char *what)
{
    const long long n = (long long)low.size();
    const long long n_words = (n + kLowWordWindows - 1) / kLowWordWindows;
    std::vector<uint64_t> bad((size_t)n_words, 0), rsw((size_t)n_words, 0);
    for (long long w = 0; w < n; ++w) {
        if (low[(size_t)w]) bad[(size_t)(w >> 6)] |= 1ull << (w & 63);
        if (rs[(size_t)w]) rsw[(size_t)(w >> 6)] |= 1ull << (w & 63);
    }
    const std::vector<Run> want = runs_by_loop(low, rs);
    std::vector<long long> first(want.size(), -1), last(want.size(), -1);
    long long starts_before = 0;
    for (long long i = 0; i < n_words; ++i) {
        LowEdges e;
        e.bad_prev63 = i > 0 ? bad[(size_t)i - 1] >> 63 : 0;
        e.bad_next0 = i + 1 < n_words ? bad[(size_t)i + 1] & 1ull : 0;
        e.rs_next0 = i + 1 < n_words ? rsw[(size_t)i + 1] & 1ull : 0;
        const uint64_t b = bad[(size_t)i], r = rsw[(size_t)i];
        CHECK((b & ~low_valid_mask(i, n)) == 0, "%s: word %lld has bits behind the array", what, i);
        uint64_t st = low_starts(b, r, e), en = low_ends(b, r, e);
        const uint64_t open = low_open_at_edge(b, r, e);
        CHECK(open <= 1, "%s: open %llu", what, (unsigned long long)open);
        // by the loop: the word's first window continues a run iff it and its left neighbour are low and it begins no read
        const long long w0 = i * kLowWordWindows;
        const bool open_want = w0 > 0 && low[(size_t)w0] && low[(size_t)w0 - 1] && !rs[(size_t)w0];
        CHECK((open != 0) == open_want, "%s: word %lld open %d want %d", what, i, (int)open, (int)open_want);
        long long ks = starts_before, ke = starts_before - (long long)open;
        starts_before += __builtin_popcountll(st);
        while (st) {
            const int bit = __builtin_ctzll(st);
            st &= st - 1;
            CHECK(ks >= 0 && ks < (long long)want.size(), "%s: start rank %lld of %zu", what, ks, want.size());
            if (ks >= 0 && ks < (long long)want.size()) first[(size_t)ks] = w0 + bit;
            ++ks;
        }
        while (en) {
            const int bit = __builtin_ctzll(en);
            en &= en - 1;
            CHECK(ke >= 0 && ke < (long long)want.size(), "%s: end rank %lld of %zu", what, ke, want.size());
            if (ke >= 0 && ke < (long long)want.size()) {
                CHECK(last[(size_t)ke] == -1, "%s: end rank %lld written twice", what, ke);
                last[(size_t)ke] = w0 + bit;
            }
            ++ke;
        }
    }
    CHECK(starts_before == (long long)want.size(), "%s: %lld starts, %zu runs", what, starts_before, want.size());
    for (size_t k = 0; k < want.size(); ++k)
        CHECK(first[k] == want[k].first && last[k] == want[k].last, "%s: run %zu is %lld..%lld, want %lld..%lld", what, k, first[k], last[k],
              want[k].first, want[k].last);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

} // namespace

int main()
{
    // exhaustive: every pattern of low and read-start bits on K windows around the boundary of two words (the other windows of the
    // two words: not low / all low), with the array ending at every length that keeps the K windows
    const int K = 5;
    for (int fill = 0; fill < 2; ++fill)
        for (int tail = 0; tail <= 3; ++tail)
            for (unsigned lowbits = 0; lowbits < (1u << K); ++lowbits)
                for (unsigned rsbits = 0; rsbits < (1u << K); ++rsbits) {
                    const long long n = 64 + (K - 2) + tail * 21;           // windows 61..65 are the K: two words, the second partial or whole
                    std::vector<int> low((size_t)n, fill), rs((size_t)n, 0);
                    rs[0] = 1;
                    for (int i = 0; i < K; ++i) { low[(size_t)(61 + i)] = (lowbits >> i) & 1; rs[(size_t)(61 + i)] = (rsbits >> i) & 1; }
                    check_array(low, rs, "exhaustive");
                }
    // small widths, exhaustively, as whole arrays of 1..8 windows
    for (int n = 1; n <= 8; ++n)
        for (unsigned lowbits = 0; lowbits < (1u << n); ++lowbits)
            for (unsigned rsbits = 1; rsbits < (1u << n); rsbits += 2) {
                std::vector<int> low((size_t)n), rs((size_t)n);
                for (int i = 0; i < n; ++i) { low[(size_t)i] = (lowbits >> i) & 1; rs[(size_t)i] = (rsbits >> i) & 1; }
                check_array(low, rs, "small");
            }
    // random words at several densities, arrays of every residue modulo 64 in their last word
    for (int it = 0; it < 4000; ++it) {
        const long long n = 1 + (long long)(rnd() % 700);
        const int dl = (int)(rnd() % 5), dr = (int)(rnd() % 6);
        std::vector<int> low((size_t)n), rs((size_t)n);
        for (long long w = 0; w < n; ++w) {
            const uint64_t x = rnd();
            low[(size_t)w] = dl == 0 ? 1 : dl == 1 ? (int)(w & 1) : (int)((x & 0xff) < (unsigned)(40 * dl));
            rs[(size_t)w] = dr == 0 ? 1 : (int)(((x >> 8) & 0xff) < (unsigned)(dr * dr * 4));
        }
        rs[0] = 1;
        check_array(low, rs, "random");
    }
    // the last word's mask
    CHECK(low_valid_mask(0, 64) == ~0ull && low_valid_mask(0, 1) == 1ull && low_valid_mask(1, 64) == 0ull && low_valid_mask(1, 65) == 1ull &&
              low_valid_mask(0, 63) == (~0ull >> 1) && low_valid_mask(5, 0) == 0ull && low_valid_mask((1ll << 40), (1ll << 46) + 3) == 7ull,
          "valid mask");
    // class bits and the uncovered bit
    CHECK(low_run_class(0, 9, 10) == (kLowHead | kLowTail) && low_run_class(0, 0, 1) == (kLowHead | kLowTail) && low_run_class(0, 3, 10) == kLowHead &&
              low_run_class(4, 9, 10) == kLowTail && low_run_class(1, 8, 10) == kLowInterior, "classes");
    CHECK(!low_uncovered(800, 1000, 800) && low_uncovered(801, 1000, 800) && !low_uncovered(799, 1000, 800) && !low_uncovered(0, 1000, 0) &&
              low_uncovered(1, 1000, 0) && !low_uncovered(1000, 1000, 1000) && !low_uncovered(0, 0, 0) &&
              low_uncovered(2147483647ll, 2147483647ll, 999) && !low_uncovered(2147483647ll, 2147483647ll, 1000), "uncovered");
    if (failures) { printf("low_cov_bits_check: %d FAILED\n", failures); return 1; }
    printf("low_cov_bits_check: ok\n");
    return 0;
}
