// containment_walk.cpp -- the yardstick of tools/containment_probe.py: the containment forest of include/raft_hip_ctn.h walked
// sequentially on one host thread, over the rule of raft_amd/csrc/containment_rule.hpp: one pass over the records for key1, one for
// key2, then every read up its chain of parents with the places composed on the way (memoised: a read after its parent).
//
//   containment_walk FILE [REPEATS]
//
// FILE: int64 n_reads, n_rec, max_overhang, min_ratio_permille, symmetric; read_len (int32 [n_reads]); qid, qs, qe, tid, ts, te
// (int32 [n_rec] each); strand (uint8 [n_rec]).  Prints one line:
//   WALK n_rec views not_longer with_parent greatest_depth checksum seconds...
// (the seconds of every repeat, reading the file not; the checksum is the sum over the reads r of
// (root[r] + root_pos[r] + depth[r] + root_rev[r]) * ((r & 1023) + 1)).
#include "../raft_amd/csrc/containment_rule.hpp"

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
    int64_t head[5];
    if (fread(head, 8, 5, f) != 5 || head[0] < 0 || head[1] < 0) return 2;
    const size_t n_reads = (size_t)head[0], n_rec = (size_t)head[1];
    const int32_t H = (int32_t)head[2], F = (int32_t)head[3];
    const bool symmetric = head[4] != 0;
    std::vector<int32_t> len, col[6];
    std::vector<uint8_t> strand;
    bool ok = read_all(f, len, n_reads);
    for (auto &c : col) ok = ok && read_all(f, c, n_rec);
    ok = ok && read_all(f, strand, n_rec);
    fclose(f);
    if (!ok) return 2;
    const int repeats = argc > 2 ? atoi(argv[2]) : 1;
    std::vector<double> seconds;
    long long views = 0, not_longer = 0, with_parent = 0, greatest = 0, checksum = 0;
    for (int rep = 0; rep < repeats; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint64_t> key1(n_reads, 0), key2(n_reads, 0);
        views = not_longer = with_parent = greatest = checksum = 0;
        for (int pass = 1; pass <= 2; ++pass)
            for (size_t i = 0; i < n_rec; ++i) {
                const int32_t q = col[0][i], t = col[3][i];
                if ((uint32_t)q >= n_reads || (uint32_t)t >= n_reads) return 3;
                const bool rev = strand[i] != 0;
                const int kind = ends_kind(q, col[1][i], col[2][i], len[q], t, col[4][i], col[5][i], len[t], rev, H, F);
                const bool from_query = kind == kEndQueryContained, from_target = kind == kEndTargetContained && !symmetric;
                if (!from_query && !from_target) continue;
                const CtnView w = from_query ? ctn_query_view(q, col[1][i], col[2][i], t, col[4][i], col[5][i])
                                             : ctn_target_view(q, col[1][i], col[2][i], t, col[4][i], col[5][i]);
                const int32_t lr = len[w.r], lc = len[w.c];
                const bool fits = ctn_acceptable(lr, w.r, lc, w.c);
                if (pass == 1) {
                    ++views;
                    if (!fits) { ++not_longer; continue; }
                    const uint64_t k = ctn_key1(lc, w.c);
                    if (k > key1[w.r]) key1[w.r] = k;
                } else if (fits && ctn_key1_parent(key1[w.r]) == w.c) {
                    const uint64_t k = ctn_view_key2(w, lr, lc, rev);
                    if (k > key2[w.r]) key2[w.r] = k;
                }
            }
        // up the chains: a stack of the reads whose parent is not placed yet
        std::vector<int32_t> root(n_reads), root_pos(n_reads, 0), depth(n_reads, -1), stack;
        std::vector<uint8_t> root_rev(n_reads, 0);
        for (size_t r0 = 0; r0 < n_reads; ++r0) {
            int32_t x = (int32_t)r0;
            while (depth[x] < 0) {
                const int32_t a = ctn_key1_parent(key1[x]);
                if (a < 0) { root[x] = x; depth[x] = 0; break; }
                stack.push_back(x);
                x = a;
            }
            while (!stack.empty()) {
                const int32_t r = stack.back(), a = ctn_key1_parent(key1[r]);
                stack.pop_back();
                const CtnPlace p = ctn_compose(CtnPlace{ctn_key2_pos(key2[r]), ctn_key2_rev(key2[r])}, len[r], len[a], CtnPlace{root_pos[a], root_rev[a] != 0});
                root[r] = root[a]; root_pos[r] = p.pos; root_rev[r] = p.rev ? 1 : 0; depth[r] = depth[a] + 1;
            }
        }
        for (size_t r = 0; r < n_reads; ++r) {
            with_parent += depth[r] > 0;
            if (depth[r] > greatest) greatest = depth[r];
            checksum += ((long long)root[r] + root_pos[r] + depth[r] + root_rev[r]) * (long long)((r & 1023) + 1);
        }
        seconds.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    printf("WALK %zu %lld %lld %lld %lld %lld", n_rec, views, not_longer, with_parent, greatest, checksum);
    for (double s : seconds) printf(" %.6f", s);
    printf("\n");
    return 0;
}
