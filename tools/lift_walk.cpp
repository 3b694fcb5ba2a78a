// lift_walk.cpp -- the yardstick of tools/lift_probe.py: a record stream lifted onto a fragment table by a plain sequential walk on one
// host thread, over the rule of raft_amd/csrc/lift_rule.hpp (lift_record_brute: every pair of rows of the two reads), writing the
// eight columns raft_hip_lift_overlaps_* writes.
//
//   lift_walk FILE [REPEATS]
//
// FILE: int64 n_reads, n_frag, n_rec, min_len; frag_offset (int64 [n_reads + 1]); frag_begin, frag_end (int32 [n_frag]); qid, qs, qe,
// tid, ts, te (int32 [n_rec] each); strand (uint8 [n_rec]).  Prints one line:
//   WALK n_rec n_out records_none records_cut pairs_dropped most_per_record checksum seconds...
// (the seconds of every repeat, reading the file not; the checksum is the sum of all output coordinates and rows).
#include "../raft_amd/csrc/lift_rule.hpp"

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
    int64_t head[4];
    if (fread(head, 8, 4, f) != 4 || head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 1) return 2;
    const size_t n_reads = (size_t)head[0], n_frag = (size_t)head[1], n_rec = (size_t)head[2];
    const int64_t min_len = head[3];
    std::vector<int64_t> off;
    std::vector<int32_t> fb, fe, col[6];
    std::vector<uint8_t> strand;
    bool ok = read_all(f, off, n_reads + 1) && read_all(f, fb, n_frag) && read_all(f, fe, n_frag);
    for (auto &c : col) ok = ok && read_all(f, c, n_rec);
    ok = ok && read_all(f, strand, n_rec);
    fclose(f);
    if (!ok) return 2;
    const int repeats = argc > 2 ? atoi(argv[2]) : 1;
    std::vector<int32_t> out[6], src;
    std::vector<uint8_t> rev;
    std::vector<double> seconds;
    long long n_out = 0, none = 0, cut = 0, most = 0, checksum = 0;
    int64_t dropped = 0;
    for (int rep = 0; rep < repeats; ++rep) {
        for (auto &c : out) c.clear();
        src.clear(); rev.clear();
        n_out = none = cut = most = checksum = 0;
        dropped = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t r = 0; r < n_rec; ++r) {
            const bool minus = strand[r] != 0;
            const int64_t n = lift_record_brute(off.data(), fb.data(), fe.data(), col[0][r], col[1][r], col[2][r], col[3][r], col[4][r], col[5][r], minus,
                                                min_len, &dropped, [&](const LiftRecord &o) {
                                                    out[0].push_back(o.qfrag); out[1].push_back(o.qs); out[2].push_back(o.qe);
                                                    out[3].push_back(o.tfrag); out[4].push_back(o.ts); out[5].push_back(o.te);
                                                    rev.push_back(minus ? 1 : 0); src.push_back((int32_t)r);
                                                });
            n_out += n; none += n == 0; cut += n > 1; most = n > most ? n : most;
        }
        seconds.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        for (auto &c : out)
            for (int32_t v : c) checksum += v;
    }
    printf("WALK %zu %lld %lld %lld %lld %lld %lld", n_rec, n_out, none, cut, (long long)dropped, most, checksum);
    for (double s : seconds) printf(" %.6f", s);
    printf("\n");
    return 0;
}
