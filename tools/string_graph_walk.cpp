// string_graph_walk.cpp -- the yardstick of tools/string_graph_probe.py: the string graph of include/raft_hip_sg.h walked sequentially
// on one host thread, over the rule of raft_amd/csrc/string_graph_rule.hpp: the arcs of the views, one std::sort by (u, w, key), one
// pass that keeps the first of every (u, w), the rows, the reduction row by row with a binary search per (arc, via) pair, the twins.
//
//   string_graph_walk FILE [REPEATS]
//
// FILE: int64 n_reads, n_rec, max_overhang, min_ratio_permille, fuzz, symmetric; read_len (int32 [n_reads]); qid, qs, qe, tid, ts, te
// (int32 [n_rec] each); strand (uint8 [n_rec]); skip (uint8 [n_reads]).  Prints one line:
//   WALK n_rec views arcs reducible kept_edges checksum seconds...
// (the seconds of every repeat, reading the file not; the checksum is the sum over the nodes u of kept[u] * ((u & 1023) + 1)).
#include "../raft_amd/csrc/string_graph_rule.hpp"

#include <algorithm>
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
    const int32_t H = (int32_t)head[2], F = (int32_t)head[3], Z = (int32_t)head[4];
    const bool symmetric = head[5] != 0;
    std::vector<int32_t> len, col[6];
    std::vector<uint8_t> strand, skip;
    bool ok = read_all(f, len, n_reads);
    for (auto &c : col) ok = ok && read_all(f, c, n_rec);
    ok = ok && read_all(f, strand, n_rec) && read_all(f, skip, n_reads);
    fclose(f);
    if (!ok) return 2;
    const int repeats = argc > 2 ? atoi(argv[2]) : 1;
    std::vector<double> seconds;
    long long views = 0, n_arcs = 0, reducible = 0, kept_edges = 0, checksum = 0;
    for (int rep = 0; rep < repeats; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<SgArc> item;
        for (size_t i = 0; i < n_rec; ++i) {
            const int32_t q = col[0][i], t = col[3][i];
            if ((uint32_t)q >= n_reads || (uint32_t)t >= n_reads) return 3;
            const bool rev = strand[i] != 0;
            const int kind = ends_kind(q, col[1][i], col[2][i], len[q], t, col[4][i], col[5][i], len[t], rev, H, F);
            if (best_end_of(kind) < 0 || skip[q] || skip[t]) continue;
            SgArc a;
            if (sg_view_arc(kind, q, col[1][i], col[2][i], len[q], t, col[4][i], col[5][i], len[t], rev, &a)) item.push_back(a);
            if (!symmetric && sg_view_arc(ends_target_view(kind, rev), t, col[4][i], col[5][i], len[t], q, col[1][i], col[2][i], len[q], rev, &a)) item.push_back(a);
        }
        views = (long long)item.size();
        std::sort(item.begin(), item.end(), [](const SgArc &a, const SgArc &b) {
            if (a.u != b.u) return a.u < b.u;
            if (a.w != b.w) return a.w < b.w;
            return sg_key_wins(sg_key(a.u, a.w, a.ext, a.back, a.span), sg_key(b.u, b.w, b.ext, b.back, b.span));
        });
        std::vector<SgArc> arc;
        for (const SgArc &a : item)
            if (arc.empty() || arc.back().u != a.u || arc.back().w != a.w) arc.push_back(a);
        n_arcs = (long long)arc.size();
        std::vector<int64_t> row(2 * n_reads + 1, 0);
        for (const SgArc &a : arc) row[(size_t)a.u + 1] += 1;
        for (size_t x = 0; x < 2 * n_reads; ++x) row[x + 1] += row[x];
        const auto find = [&](int32_t from, int32_t to) -> int64_t {
            int64_t lo = row[(size_t)from], hi = row[(size_t)from + 1];
            const int64_t end = hi;
            while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (arc[(size_t)mid].w < to) lo = mid + 1; else hi = mid; }
            return lo < end && arc[(size_t)lo].w == to ? lo : -1;
        };
        std::vector<uint8_t> red(arc.size(), 0);
        reducible = 0;
        for (size_t u = 0; u < 2 * n_reads; ++u)
            for (int64_t a = row[u]; a < row[u + 1]; ++a)
                for (int64_t v = row[u]; v < row[u + 1] && !red[(size_t)a]; ++v) {
                    if (v == a || !(arc[(size_t)v].ext < arc[(size_t)a].ext)) continue;
                    const int64_t t = find(arc[(size_t)v].w ^ 1, arc[(size_t)a].w);
                    if (t >= 0 && sg_reducible(arc[(size_t)v].ext, arc[(size_t)t].ext, arc[(size_t)a].ext, Z)) { red[(size_t)a] = 1; reducible += 1; }
                }
        kept_edges = checksum = 0;
        for (size_t a = 0; a < arc.size(); ++a) {
            const int64_t t = find(arc[a].w, arc[a].u);
            const bool survives = !red[a] && !(t >= 0 && red[(size_t)t]);
            if (survives) checksum += (long long)((arc[a].u & 1023) + 1);
            if (survives && (t < 0 || (arc[a].u >> 1) < (arc[a].w >> 1))) kept_edges += 1;
        }
        seconds.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    printf("WALK %zu %lld %lld %lld %lld %lld", n_rec, views, n_arcs, reducible, kept_edges, checksum);
    for (double s : seconds) printf(" %.6f", s);
    printf("\n");
    return 0;
}
