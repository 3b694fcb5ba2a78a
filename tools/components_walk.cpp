// components_walk.cpp -- the yardstick of tools/components_probe.py: the connected components of include/raft_hip_cc.h by a plain
// sequential union-find on one host thread, over the rule of raft_amd/csrc/ovl_ends_rule.hpp.
//
//   components_walk FILE [REPEATS]
//
// FILE: int64 n_reads, n_rec, max_overhang, min_ratio_permille, kind_mask, symmetric; read_len (int32 [n_reads]); qid, qs, qe, tid, ts,
// te (int32 [n_rec] each); strand (uint8 [n_rec]).  Prints one line:
//   WALK n_rec edge_records components largest_reads checksum seconds...
// (the seconds of every repeat, reading the file not; the checksum is the sum over the reads r of component[r] * ((r & 1023) + 1)).
#include "../raft_amd/csrc/ovl_ends_rule.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace raft;

template <class T> static bool read_all(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[6];
    if (fread(head, 8, 6, f) != 6 || head[0] < 0 || head[1] < 0) return 2;
    const size_t n_reads = (size_t)head[0], n_rec = (size_t)head[1];
    const int32_t H = (int32_t)head[2], F = (int32_t)head[3], mask = (int32_t)head[4];
    std::vector<int32_t> len, col[6];
    std::vector<uint8_t> strand;
    bool ok = read_all(f, len, n_reads);
    for (auto &c : col) ok = ok && read_all(f, c, n_rec);
    ok = ok && read_all(f, strand, n_rec);
    fclose(f);
    if (!ok) return 2;
    const int repeats = argc > 2 ? atoi(argv[2]) : 1;
    std::vector<int32_t> parent(n_reads), component(n_reads), size(n_reads);
    std::vector<double> seconds;
    long long edges = 0, components = 0, largest = 0, checksum = 0;
    for (int rep = 0; rep < repeats; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        edges = components = largest = checksum = 0;
        for (size_t r = 0; r < n_reads; ++r) parent[r] = (int32_t)r;
        const auto find = [&](int32_t x) {
            while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
            return x;
        };
        for (size_t i = 0; i < n_rec; ++i) {
            const int32_t q = col[0][i], t = col[3][i];
            if ((uint32_t)q >= n_reads || (uint32_t)t >= n_reads) return 3;
            const int kind = ends_kind(q, col[1][i], col[2][i], len[q], t, col[4][i], col[5][i], len[t], strand[i] != 0, H, F);
            if (!((mask >> kind) & 1)) continue;
            edges += 1;
            const int32_t a = find(q), b = find(t);
            if (a != b) parent[a > b ? a : b] = a > b ? b : a;       // the smaller id stays the root
        }
        // dense ids in the order of the smallest reads: a root is its component's smallest read and comes before its members
        for (size_t r = 0; r < n_reads; ++r) {
            const int32_t top = find((int32_t)r);
            if (top == (int32_t)r) { component[r] = (int32_t)components++; size[component[r]] = 0; }
            else component[r] = component[top];
            const int32_t s = ++size[component[r]];
            largest = s > largest ? s : largest;
            checksum += (long long)component[r] * (long long)((r & 1023) + 1);
        }
        seconds.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    printf("WALK %zu %lld %lld %lld %lld", n_rec, edges, components, largest, checksum);
    for (double s : seconds) printf(" %.6f", s);
    printf("\n");
    return 0;
}
