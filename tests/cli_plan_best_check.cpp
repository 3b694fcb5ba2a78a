// cli_plan_best_check.cpp -- what `raft --best-overlaps` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a program of its own
// (tests/test_cli_plan_best.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

int main()
{
    using namespace raft_cli;
    using cli_check::usage;
    // the option needs --overlap-ends (max_overhang -1: not asked for); without the option everything goes
    CHECK(usage(-1, false, false, false, false, false) && usage(0, false, false, false, false, false) && usage(1000, false, false, false, false, false));
    CHECK(usage(0, false, true, false, false, false) && usage(1000, false, true, false, false, false) && usage(2147483647, false, true, false, false, false));
    CHECK(!usage(-1, false, true, false, false, false));
    // ... and leaves the rules of the options before it alone
    CHECK(usage(-1, false, false, false, false, false) && !usage(-1, true, false, false, false, false) && cli_check::columns(false, 0, false) == RAFT_HOST_PAF_STRAND);
    // the stdout line
    CHECK(best_overlaps_line(25236, 412, 9000, 38, 28, 8, 2, 279, 300) ==
          "INFO, best_overlaps(), records = 25236, candidates = 412, left out = 9000, ends with a best overlap = 38, mutual = 28, "
          "reads with both ends mutual = 8, reads without a best overlap = 2, reads left out = 279 of 300");
    CHECK(best_overlaps_line(0, 0, 0, 0, 0, 0, 0, 0, 0) ==
          "INFO, best_overlaps(), records = 0, candidates = 0, left out = 0, ends with a best overlap = 0, mutual = 0, "
          "reads with both ends mutual = 0, reads without a best overlap = 0, reads left out = 0 of 0");
    CHECK(best_overlaps_line(3000000000LL, 6000000000LL, 5999999999LL, 4294967294LL, 4294967292LL, 2147483646, 1, 2, 2147483647) ==
          "INFO, best_overlaps(), records = 3000000000, candidates = 6000000000, left out = 5999999999, ends with a best overlap = 4294967294, "
          "mutual = 4294967292, reads with both ends mutual = 2147483646, reads without a best overlap = 1, reads left out = 2 of 2147483647");
    return cli_check::finish("cli_plan_best_check");
}
