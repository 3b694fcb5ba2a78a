// cli_plan_lift_check.cpp -- what `raft --fragment-paf / --fragment-paf-min` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a
// program of its own (tests/test_cli_plan_lift.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

static bool min_len(const char *text, int32_t *v) { return cli_check::parsed(raft_cli::parse_fragment_paf_min, text, v); }

// Request::strand over the two options it reads
static bool strand(int32_t overlap_ends, bool fragment_paf)
{
    raft_cli::Options o;
    o.overlap_ends = overlap_ends; o.fragment_paf = fragment_paf;
    return raft_cli::request(o, false).strand;
}

int main()
{
    using namespace raft_cli;
    using cli_check::columns;
    using cli_check::keeps;
    using cli_check::usage;
    int32_t v = -7;
    // --fragment-paf-min: digits alone, 1 <= L <= INT32_MAX; the default is 1
    CHECK(kFragmentPafMinDefault == 1);
    CHECK(min_len("1", &v) && v == 1);
    CHECK(min_len("501", &v) && v == 501);
    CHECK(min_len("2147483647", &v) && v == 2147483647);
    CHECK(min_len("0500", &v) && v == 500);
    v = -7;
    const char *bad[] = {"", "0", "00", "2147483648", "99999999999999999999", "-1", "+1", " 1", "1 ", "1.0", "1e3", "2k", "x"};
    for (const char *t : bad) {
        CHECK(!min_len(t, &v));
        CHECK(v == -7);                                    // a refused text leaves the value alone
    }
    CHECK(!parse_fragment_paf_min(nullptr, &v));
    // ... and means nothing without --fragment-paf: a usage error
    CHECK(usage(-1, false, false, false, false, false) && usage(-1, false, false, false, true, false) && usage(-1, false, false, false, true, true));
    CHECK(!usage(-1, false, false, false, false, true));
    // ... and leaves the rules of the options before it alone
    CHECK(usage(0, false, true, true, false, false) && !usage(0, false, false, true, false, false) && usage(0, false, true, false, false, false) &&
          !usage(-1, false, true, false, false, false));
    CHECK(usage(-1, false, false, false, false, false) && !usage(-1, true, false, false, false, false));
    // the strand is tokenised for --overlap-ends or for the lift, fields 10 and 11 for the filter alone
    CHECK(!strand(-1, false) && strand(0, false) && strand(-1, true) && strand(1000, true));
    CHECK(columns(false, -1, false) == 0);
    CHECK(columns(false, -1, true) == RAFT_HOST_PAF_STRAND);
    CHECK(columns(false, 100, false) == RAFT_HOST_PAF_STRAND && columns(false, 100, true) == RAFT_HOST_PAF_STRAND);
    CHECK(columns(true, -1, false) == RAFT_HOST_PAF_QUALITY);
    CHECK(columns(true, -1, true) == (RAFT_HOST_PAF_QUALITY | RAFT_HOST_PAF_STRAND));
    CHECK(columns(true, 0, true) == (RAFT_HOST_PAF_QUALITY | RAFT_HOST_PAF_STRAND));
    for (int filter = 0; filter < 2; ++filter)
        for (int ends = -1; ends < 2; ++ends)                // without the option: the mask the job had
            CHECK(columns(filter != 0, ends, false) == ((filter ? RAFT_HOST_PAF_QUALITY : 0) | (ends >= 0 ? RAFT_HOST_PAF_STRAND : 0)));
    // the query ids are kept past prepare_input for the lift as for --fragment-overlaps
    CHECK(!keeps(false, 0, false, true) && !keeps(true, 0, false, false));
    CHECK(keeps(true, 0, false, true) && keeps(true, 0, true, false) && keeps(true, 1000, false, false));
    for (int prepare = 0; prepare < 2; ++prepare)
        for (int anchor = 0; anchor < 2; ++anchor)
            for (int frag = 0; frag < 2; ++frag)             // without the option: what the job kept
                CHECK(keeps(prepare != 0, anchor, frag != 0, false) == (prepare != 0 && (anchor > 0 || frag != 0)));
    // the stdout line
    CHECK(fragment_paf_line(1, 25236, 31002, 5112, 17, 3, 6) ==
          "INFO, fragment_paf(), min_len = 1, records = 25236, lifted = 31002, cut = 5112, without a fragment pair = 17, dropped pairs = 3, "
          "most from one record = 6");
    CHECK(fragment_paf_line(501, 0, 0, 0, 0, 0, 0) ==
          "INFO, fragment_paf(), min_len = 501, records = 0, lifted = 0, cut = 0, without a fragment pair = 0, dropped pairs = 0, most from one record = 0");
    CHECK(fragment_paf_line(2147483647, 1073741823, 2147483646, 1073741822, 1, 4611686018427387903LL, 1600) ==
          "INFO, fragment_paf(), min_len = 2147483647, records = 1073741823, lifted = 2147483646, cut = 1073741822, without a fragment pair = 1, "
          "dropped pairs = 4611686018427387903, most from one record = 1600");
    return cli_check::finish("cli_plan_lift_check");
}
