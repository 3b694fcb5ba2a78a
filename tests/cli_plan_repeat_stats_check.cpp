// cli_plan_repeat_stats_check.cpp -- the decisions `raft --repeat-stats` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a
// program of its own (tests/test_cli_plan_repeat_stats.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

// Request::survey and Request::repeat_stats_second_pass over the four options they read
static raft_cli::Request asked(bool auto_cov, bool read_stats, int32_t low_cov, bool repeat_stats)
{
    raft_cli::Options o;
    o.auto_cov = auto_cov; o.read_stats = read_stats; o.low_cov = low_cov; o.repeat_stats = repeat_stats;
    return raft_cli::request(o, false);
}

int main()
{
    using namespace raft_cli;
    using cli_check::keeps;
    // the survey runs for -e auto, --read-stats, --low-cov C (C >= 0; -1: not asked for) -- and for --repeat-stats alone
    CHECK(!asked(false, false, -1, false).survey);
    CHECK(asked(true, false, -1, false).survey && asked(false, true, -1, false).survey && asked(false, false, 0, false).survey);
    CHECK(asked(false, false, -1, true).survey && asked(true, true, 5, true).survey);
    // with -e N the survey pass is the stats pass; with -e auto one more runs under the estimate -- only when the table is asked for
    CHECK(!asked(false, false, -1, true).repeat_stats_second_pass && asked(true, false, -1, true).repeat_stats_second_pass);
    CHECK(!asked(true, false, -1, false).repeat_stats_second_pass && !asked(false, false, -1, false).repeat_stats_second_pass);
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
    CHECK(!keeps(true, 0, false, false) && keeps(true, 1, false, false) && keeps(true, 0, true, false) && !keeps(false, 1, true, false));
    for (int other = 0; other < 8; ++other) {                // ... whatever else is asked for beside it
        Options o;
        o.repeat_stats = true; o.auto_cov = other & 1; o.read_stats = (other & 2) != 0; o.low_cov = (other & 4) ? 3 : -1;
        CHECK(!request(o, true).keep_query_ids && !request(o, false).keep_query_ids);
    }
    return cli_check::finish("cli_plan_repeat_stats_check");
}
