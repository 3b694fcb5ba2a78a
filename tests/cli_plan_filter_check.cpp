// cli_plan_filter_check.cpp -- what `raft --min-identity / --min-overlap` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a
// program of its own (tests/test_cli_plan_filter.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

static bool identity(const char *text, int32_t *v) { return cli_check::parsed(raft_cli::parse_min_identity, text, v); }
static bool overlap(const char *text, int32_t *v) { return cli_check::parsed(raft_cli::parse_min_overlap, text, v); }

// Request::filter over the two options it reads
static bool filters(int32_t permille, int32_t min_span)
{
    raft_cli::Options o;
    o.min_identity = permille; o.min_overlap = min_span;
    return raft_cli::request(o, false).filter;
}

int main()
{
    using namespace raft_cli;
    int32_t v = -7;
    // --min-identity: digits with at most one decimal digit, 0 < PCT <= 100, into per mille
    CHECK(identity("99", &v) && v == 990);
    CHECK(identity("99.5", &v) && v == 995);
    CHECK(identity("100", &v) && v == 1000);
    CHECK(identity("0.1", &v) && v == 1);
    CHECK(identity("100.0", &v) && v == 1000);
    CHECK(identity("1", &v) && v == 10);
    CHECK(identity("099.9", &v) && v == 999);
    CHECK(identity("7.0", &v) && v == 70);
    v = -7;
    const char *bad[] = {"", "0", "100.1", "99.55", "1e2", "-1", " 99", "99.", "0.0", "00", "101", "1000", "99999999999999999999", ".5", "99 ", "99.5 ",
                         "+99", "9,5", "99..5", "99.x", "x", "0x10", "1.", "4294967395", "99.5.1"};
    for (const char *t : bad) {
        CHECK(!identity(t, &v));
        CHECK(v == -7);                                    // a refused text leaves the value alone
    }
    CHECK(!parse_min_identity(nullptr, &v));
    // --min-overlap: digits alone, 1 <= BASES <= INT32_MAX
    CHECK(overlap("1", &v) && v == 1);
    CHECK(overlap("2000", &v) && v == 2000);
    CHECK(overlap("2147483647", &v) && v == 2147483647);
    CHECK(overlap("0500", &v) && v == 500);
    v = -7;
    const char *bad_overlap[] = {"", "0", "00", "2147483648", "99999999999999999999", "-1", "+1", " 1", "1 ", "1.0", "1e3", "2k", "x"};
    for (const char *t : bad_overlap) {
        CHECK(!overlap(t, &v));
        CHECK(v == -7);
    }
    CHECK(!parse_min_overlap(nullptr, &v));
    // either option makes the job filter
    CHECK(!filters(0, 0) && filters(990, 0) && filters(0, 1) && filters(1000, 2147483647));
    // the stdout line
    CHECK(filter_overlaps_line(990, 0, 300, 200, 100, 0) ==
          "INFO, filter_overlaps(), min_identity = 990 per mille, min_overlap = 0, records = 300, kept = 200, below identity = 100, below overlap = 0");
    CHECK(filter_overlaps_line(0, 500, 0, 0, 0, 0) ==
          "INFO, filter_overlaps(), min_identity = 0 per mille, min_overlap = 500, records = 0, kept = 0, below identity = 0, below overlap = 0");
    CHECK(filter_overlaps_line(995, 2147483647, 3000000000LL, 1, 2999999999LL, 2999999998LL) ==
          "INFO, filter_overlaps(), min_identity = 995 per mille, min_overlap = 2147483647, records = 3000000000, kept = 1, below identity = 2999999999, "
          "below overlap = 2999999998");
    return cli_check::finish("cli_plan_filter_check");
}
