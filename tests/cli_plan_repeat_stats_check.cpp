// cli_plan_repeat_stats_check.cpp -- the decisions `raft --repeat-stats` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a
// program of its own (tests/test_cli_plan_repeat_stats.py builds it under the address and undefined-behaviour sanitizers).
#include "../raft_amd/host/cli_plan.hpp"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

int main()
{
    using namespace raft_cli;
    // the survey runs for -e auto, --read-stats, --low-cov C (C >= 0; -1: not asked for) -- and for --repeat-stats alone
    CHECK(!survey_needed(false, false, -1, false));
    CHECK(survey_needed(true, false, -1, false) && survey_needed(false, true, -1, false) && survey_needed(false, false, 0, false));
    CHECK(survey_needed(false, false, -1, true) && survey_needed(true, true, 5, true));
    // with -e N the survey pass is the stats pass; with -e auto one more runs under the estimate -- only when the table is asked for
    CHECK(!repeat_stats_second_pass(false, true) && repeat_stats_second_pass(true, true));
    CHECK(!repeat_stats_second_pass(true, false) && !repeat_stats_second_pass(false, false));
    // threshold = max((int)(est_cov * cov_mul), 1): truncated as the job's high_cov is
    CHECK(repeat_stats_threshold(30, 1.5) == 45 && repeat_stats_threshold(3, 1.5) == 4 && repeat_stats_threshold(1, 1.5) == 1);
    CHECK(repeat_stats_threshold(1, 0.4) == 1 && repeat_stats_threshold(2, 0.4) == 1 && repeat_stats_threshold(5, 0.4) == 2);
    CHECK(repeat_stats_threshold(7, 1.0) == 7 && repeat_stats_threshold(1000000, 2.0) == 2000000);
    // the stdout line: untouched is the runs without a touching side
    CHECK(repeat_stats_line(10, 6, 4, 3, 8, 25) ==
          "INFO, repeat_stats(), repeats = 10, interior = 6, spanned = 4, interior spanned = 3, untouched = 2, sides inside a repeat = 25");
    CHECK(repeat_stats_line(0, 0, 0, 0, 0, 0) ==
          "INFO, repeat_stats(), repeats = 0, interior = 0, spanned = 0, interior spanned = 0, untouched = 0, sides inside a repeat = 0");
    CHECK(repeat_stats_line(3000000000LL, 1, 2, 1, 3000000000LL, 9000000000LL) ==
          "INFO, repeat_stats(), repeats = 3000000000, interior = 1, spanned = 2, interior spanned = 1, untouched = 0, sides inside a repeat = 9000000000");
    // the options that read the query ids after the job are what they were: this one reads them before prepare_input()
    CHECK(!keeps_query_ids(true, 0, false) && keeps_query_ids(true, 1, false) && keeps_query_ids(true, 0, true) && !keeps_query_ids(false, 1, true));
    printf("cli_plan_repeat_stats_check: ok\n");
    return 0;
}
