// unitig_walk.cpp -- the yardstick of tools/unitigs_probe.py: the unitigs of a table of best overlaps by a plain sequential walk on one
// host thread, over the rule of raft_amd/csrc/unitig_rule.hpp, writing every array raft_hip_unitigs_* writes.
//
//   unitig_walk TABLE [REPEATS]
//
// TABLE: int32 n_reads, then read_len (int32 [n]), partner (int32 [2n]), span (int32 [2n]), flags (uint8 [n]).  Prints one line:
//   WALK n_reads unitigs singletons circular longest_reads longest_length total_length skipped seconds...
// (the seconds of every repeat, the consistency check included, reading the file not).
#include "../raft_amd/csrc/unitig_rule.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace raft;

struct Start { int32_t read, half; bool circular; };

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    std::vector<int32_t> len((size_t)n), partner(2 * (size_t)n), span(2 * (size_t)n);
    std::vector<uint8_t> flags((size_t)n);
    if (fread(len.data(), 4, (size_t)n, f) != (size_t)n || fread(partner.data(), 4, 2 * (size_t)n, f) != 2 * (size_t)n ||
        fread(span.data(), 4, 2 * (size_t)n, f) != 2 * (size_t)n || fread(flags.data(), 1, (size_t)n, f) != (size_t)n)
        return 2;
    fclose(f);
    const int repeats = argc > 2 ? atoi(argv[2]) : 1;
    const auto succ = [&](int32_t h) { return utg_succ(partner.data(), flags.data(), utg_read(h), utg_end(h)); };
    std::vector<double> seconds;
    long long unitigs = 0, singletons = 0, circular = 0, longest_reads = 0, longest_length = 0, total_length = 0, skipped = 0;
    for (int rep = 0; rep < repeats; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int32_t r = 0; r < n; ++r)
            for (int e = 0; e < 2; ++e)
                if (!utg_end_ok(n, len.data(), partner.data(), span.data(), flags.data(), r, e)) { printf("inconsistent at read %d\n", r); return 1; }
        std::vector<int32_t> unitig((size_t)n, -1), index((size_t)n, -1), order, utg_reads;
        std::vector<int64_t> offset((size_t)n, 0), utg_off(1, 0), utg_length;
        std::vector<uint8_t> orient((size_t)n, 0), utg_circular, seen((size_t)n, 0);
        std::vector<Start> starts;
        order.reserve((size_t)n);
        skipped = 0;
        for (int32_t r = 0; r < n; ++r) {
            if (utg_skipped(flags[r])) { skipped += 1; continue; }
            if (seen[r]) continue;
            seen[r] = 1;
            int32_t term[2] = {0, 0};
            bool cyc = false;
            for (int e = 0; e < 2 && !cyc; ++e) {
                int32_t h = utg_half(r, e);
                for (int32_t nx = succ(h); nx != kUtgNil; nx = succ(h)) {
                    h = nx;
                    if (utg_read(h) == r) { cyc = true; break; }
                    seen[utg_read(h)] = 1;
                }
                term[e] = h;
            }
            if (cyc || utg_read(term[0]) == utg_read(term[1])) starts.push_back({r, utg_half(r, 1), cyc});
            else {
                const int32_t free_half = utg_read(term[0]) < utg_read(term[1]) ? term[0] : term[1];
                starts.push_back({utg_read(free_half), utg_twin(free_half), false});
            }
        }
        std::sort(starts.begin(), starts.end(), [](const Start &a, const Start &b) { return a.read < b.read; });
        unitigs = (long long)starts.size(); singletons = circular = longest_reads = longest_length = total_length = 0;
        for (size_t u = 0; u < starts.size(); ++u) {
            int32_t h = starts[u].half, k = 0;
            int64_t off = 0, length = 0;
            for (;;) {
                const int32_t r = utg_read(h);
                unitig[r] = (int32_t)u; index[r] = k++; offset[r] = off; orient[r] = (uint8_t)(1 - utg_end(h));
                order.push_back(r);
                const int32_t nx = succ(h);
                if (nx == kUtgNil) { length = off + utg_len(len[r]); break; }
                off += (int64_t)utg_len(len[r]) - span[h];
                if (starts[u].circular && utg_read(nx) == starts[u].read) { length = off; break; }
                h = nx;
            }
            utg_off.push_back((int64_t)order.size()); utg_reads.push_back(k); utg_length.push_back(length); utg_circular.push_back(starts[u].circular);
            singletons += k == 1; circular += starts[u].circular; total_length += length;
            longest_reads = std::max<long long>(longest_reads, k); longest_length = std::max<long long>(longest_length, length);
        }
        seconds.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        if (order.size() + (size_t)skipped != (size_t)n) return 1;
    }
    printf("WALK %d %lld %lld %lld %lld %lld %lld %lld", n, unitigs, singletons, circular, longest_reads, longest_length, total_length, skipped);
    for (double s : seconds) printf(" %.6f", s);
    printf("\n");
    return 0;
}
