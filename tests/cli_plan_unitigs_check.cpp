// cli_plan_unitigs_check.cpp -- what `raft --unitigs` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a program of its own
// (tests/test_cli_plan_unitigs.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

#include <vector>

static int64_t n50(std::vector<int64_t> v) { return raft_cli::unitig_n50(v.data(), (int64_t)v.size()); }

int main()
{
    using namespace raft_cli;
    using cli_check::usage;
    // the option needs --best-overlaps; without the option everything goes
    CHECK(usage(0, false, false, false, false, false) && usage(0, false, true, false, false, false) && usage(0, false, true, true, false, false));
    CHECK(!usage(0, false, false, true, false, false));
    // ... and leaves the rules of the options before it alone
    CHECK(usage(0, false, true, false, false, false) && !usage(-1, false, true, false, false, false) && usage(-1, false, false, false, false, false) &&
          !usage(-1, true, false, false, false, false));
    // N50: no unitigs, one, ties, the exact half, just below it, any order, lengths of 0, totals beyond 2^32
    CHECK(unitig_n50(nullptr, 0) == 0 && n50({}) == 0);
    CHECK(n50({7}) == 7 && n50({0}) == 0);
    CHECK(n50({5, 5, 5, 5}) == 5 && n50({3, 9, 9, 3}) == 9);
    CHECK(n50({10, 6, 4}) == 10);                          // 2 * 10 == 20: the first prefix that holds half
    CHECK(n50({10, 6, 5}) == 6);                           // 2 * 10 < 21
    CHECK(n50({4, 10, 6}) == 10 && n50({5, 6, 10}) == 6);
    CHECK(n50({0, 0, 0}) == 0 && n50({0, 8, 0}) == 8);
    CHECK(n50({1, 1, 1, 1, 1, 1, 7}) == 7 && n50({1, 1, 1, 1, 1, 1, 1, 7}) == 7 && n50({1, 1, 1, 1, 1, 1, 1, 1, 7}) == 1);
    CHECK(n50({4294967296LL, 4294967296LL, 3}) == 4294967296LL);
    CHECK(n50({6000000000LL, 5000000000LL, 4000000000LL, 1}) == 5000000000LL);
    CHECK(n50({4611686018427387904LL / 4, 4611686018427387904LL / 4, 4611686018427387904LL / 4 + 1}) == 4611686018427387904LL / 4);
    {
        const std::vector<int64_t> v = {2, 1, 3, 1};
        std::vector<int64_t> copy = v;
        CHECK(unitig_n50(copy.data(), 4) == 2 && copy == v);          // the caller's array stays as it is
        CHECK(unitig_n50(copy.data(), 3) == 3 && unitig_n50(copy.data(), 2) == 2 && unitig_n50(copy.data(), -1) == 0);
    }
    // the stdout line
    CHECK(unitigs_line(46, 1, 3, 1, 1, 40, 122377, 137377, 122377) ==
          "INFO, unitigs(), reads = 46, left out = 1, unitigs = 3, singletons = 1, circular = 1, longest = 40 reads, longest length = 122377, "
          "total length = 137377, N50 = 122377");
    CHECK(unitigs_line(0, 0, 0, 0, 0, 0, 0, 0, 0) ==
          "INFO, unitigs(), reads = 0, left out = 0, unitigs = 0, singletons = 0, circular = 0, longest = 0 reads, longest length = 0, "
          "total length = 0, N50 = 0");
    CHECK(unitigs_line(1073741823, 2, 3000000, 2999999, 7, 1073741820, 2305843009213693951LL, 4611686018427387903LL, 4294967296LL) ==
          "INFO, unitigs(), reads = 1073741823, left out = 2, unitigs = 3000000, singletons = 2999999, circular = 7, longest = 1073741820 reads, "
          "longest length = 2305843009213693951, total length = 4611686018427387903, N50 = 4294967296");
    return cli_check::finish("cli_plan_unitigs_check");
}
