// cli_plan_ends_check.cpp -- what `raft --overlap-ends / --ends-min-ratio` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a
// program of its own (tests/test_cli_plan_ends.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

int main()
{
    using namespace raft_cli;
    using cli_check::columns;
    using cli_check::parsed;
    using cli_check::usage;
    int32_t v = -7;
    // --overlap-ends H: digits alone, 0 .. INT32_MAX
    CHECK(parsed(parse_overlap_ends, "0", &v) && v == 0);
    CHECK(parsed(parse_overlap_ends, "1000", &v) && v == 1000);
    CHECK(parsed(parse_overlap_ends, "2147483647", &v) && v == 2147483647);
    CHECK(parsed(parse_overlap_ends, "0100", &v) && v == 100);
    CHECK(parsed(parse_overlap_ends, "00", &v) && v == 0);
    v = -7;
    const char *bad_h[] = {"", "2147483648", "99999999999999999999", "-1", "+1", " 1", "1 ", "1.0", "1e3", "2k", "x", "0x10", "auto"};
    for (const char *t : bad_h) {
        CHECK(!parsed(parse_overlap_ends, t, &v));
        CHECK(v == -7);                                    // a refused text leaves the value alone
    }
    CHECK(!parse_overlap_ends(nullptr, &v));
    // --ends-min-ratio F: digits alone, 0 .. 1000
    CHECK(parsed(parse_ends_min_ratio, "0", &v) && v == 0);
    CHECK(parsed(parse_ends_min_ratio, "800", &v) && v == 800);
    CHECK(parsed(parse_ends_min_ratio, "1000", &v) && v == 1000);
    CHECK(parsed(parse_ends_min_ratio, "0999", &v) && v == 999);
    v = -7;
    const char *bad_f[] = {"", "1001", "2147483647", "2147483648", "99999999999999999999", "-1", "+800", " 800", "800 ", "80.0", "0.8", "8e2", "x", "80%"};
    for (const char *t : bad_f) {
        CHECK(!parsed(parse_ends_min_ratio, t, &v));
        CHECK(v == -7);
    }
    CHECK(!parse_ends_min_ratio(nullptr, &v));
    CHECK(kEndsMinRatioDefault == 800);
    // the second option needs the first (max_overhang -1: not asked for)
    CHECK(usage(-1, false, false, false, false, false) && usage(0, false, false, false, false, false) && usage(0, true, false, false, false, false) &&
          usage(2147483647, true, false, false, false, false));
    CHECK(!usage(-1, true, false, false, false, false));
    // the columns the tokeniser is asked for
    CHECK(columns(false, -1, false) == 0 && columns(true, -1, false) == RAFT_HOST_PAF_QUALITY && columns(false, 0, false) == RAFT_HOST_PAF_STRAND);
    CHECK(columns(true, 0, false) == (RAFT_HOST_PAF_QUALITY | RAFT_HOST_PAF_STRAND) && RAFT_HOST_PAF_QUALITY == 1 && RAFT_HOST_PAF_STRAND == 2);
    // the stdout line
    CHECK(overlap_ends_line(1000, 800, 300, 100, 20, 30, 140, 4, 6, 25, 7, 3, 40) ==
          "INFO, overlap_ends(), max_overhang = 1000, min_ratio = 800 per mille, records = 300, internal = 100, query contained = 20, target contained = 30, "
          "dovetail = 140, self = 4, invalid = 6, contained reads = 25, dead ends = 7, isolated reads = 3 of 40");
    CHECK(overlap_ends_line(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) ==
          "INFO, overlap_ends(), max_overhang = 0, min_ratio = 0 per mille, records = 0, internal = 0, query contained = 0, target contained = 0, "
          "dovetail = 0, self = 0, invalid = 0, contained reads = 0, dead ends = 0, isolated reads = 0 of 0");
    CHECK(overlap_ends_line(2147483647, 1000, 3000000000LL, 2999999999LL, 1, 2, 3, 4, 5, 6, 7, 8, 2147483647) ==
          "INFO, overlap_ends(), max_overhang = 2147483647, min_ratio = 1000 per mille, records = 3000000000, internal = 2999999999, query contained = 1, "
          "target contained = 2, dovetail = 3, self = 4, invalid = 5, contained reads = 6, dead ends = 7, isolated reads = 8 of 2147483647");
    return cli_check::finish("cli_plan_ends_check");
}
