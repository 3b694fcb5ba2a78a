// low_cov_bits.hpp -- the word arithmetic of the low-coverage runs (low_cov.hpp) as plain functions: no HIP call and no HIP header,
// so a host compiler alone builds it (tests/low_cov_bits_check.cpp does, under the sanitizers); the kernels call the same functions.
//
// Two bitmaps over the concatenated windows, 64 windows per word, window w in bit (w & 63) of word (w >> 6):
//     bad : window w is low (cov[w] <= low_cov); 0 from the array's last window on
//     rs  : window w is the first window of a read
// A run is a maximal sequence of consecutive low windows of ONE read, so a run starts at a low window whose left neighbour is not
// low or which begins a read, and ends at a low window whose right neighbour is not low or begins a read.  Every run has exactly
// one start and one end and runs do not nest: the k-th start bit and the k-th end bit of the array belong to the same run.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RAFT_LOW_HD __host__ __device__ inline
#else
#define RAFT_LOW_HD inline
#endif

namespace raft {

constexpr int kLowWordWindows = 64;     // windows of one bitmap word

// What a word needs from its neighbours: bit 63 of the word before (0 for the first word), bit 0 of the word behind (bad: 0 for
// the last word; rs: anything there, since bad is 0 behind the array's last window).
struct LowEdges { uint64_t bad_prev63, bad_next0, rs_next0; };

// windows of word `word` that exist: all 64, or the low n_bins % 64 bits in the array's last, partial word, or none
RAFT_LOW_HD uint64_t low_valid_mask(long long word, long long n_bins)
{
    const long long left = n_bins - word * kLowWordWindows;
    return left >= kLowWordWindows ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
}

RAFT_LOW_HD uint64_t low_starts(uint64_t bad, uint64_t rs, const LowEdges &e)
{
    return bad & (~((bad << 1) | (e.bad_prev63 & 1ull)) | rs);
}

RAFT_LOW_HD uint64_t low_ends(uint64_t bad, uint64_t rs, const LowEdges &e)
{
    const uint64_t bad_right = (bad >> 1) | ((e.bad_next0 & 1ull) << 63);      // bit i: window i + 1 is low
    const uint64_t rs_right = (rs >> 1) | ((e.rs_next0 & 1ull) << 63);         // bit i: window i + 1 begins a read
    return bad & (~bad_right | rs_right);
}

// 1 when a run that began in an earlier word goes on into this word's first window: the word's first end bit then closes a run
// whose start bit lies before the word
RAFT_LOW_HD uint64_t low_open_at_edge(uint64_t bad, uint64_t rs, const LowEdges &e)
{
    return bad & ~rs & e.bad_prev63 & 1ull;
}

// low_flags of a read
constexpr unsigned kLowInterior = 1u, kLowHead = 2u, kLowTail = 4u, kLowUncovered = 8u;

// the class bits of one run j1..j2 of a read of n_windows windows
RAFT_LOW_HD unsigned low_run_class(long long j1, long long j2, long long n_windows)
{
    unsigned f = 0;
    if (j1 == 0) f |= kLowHead;
    if (j2 == n_windows - 1) f |= kLowTail;
    if (j1 > 0 && j2 < n_windows - 1) f |= kLowInterior;
    return f;
}

// bit 3: more than uncovered_permille thousandths of the read's bases lie in low runs (64-bit integers: 1000 * 2^31 fits)
RAFT_LOW_HD bool low_uncovered(long long low_bases, long long len, long long uncovered_permille)
{
    return 1000ll * low_bases > uncovered_permille * len;
}

} // namespace raft
