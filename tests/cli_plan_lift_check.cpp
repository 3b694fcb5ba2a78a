// cli_plan_lift_check.cpp -- what `raft --fragment-paf / --fragment-paf-min` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a
// program of its own (tests/test_cli_plan_lift.py builds it under the address and undefined-behaviour sanitizers).
#include "../raft_amd/host/cli_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }    \
    } while (0)

// the text in a heap block of exactly its size, so that a read behind its end is the sanitizer's
static bool min_len(const char *text, int32_t *v)
{
    char *copy = (char *)malloc(strlen(text) + 1);
    strcpy(copy, text);
    const bool ok = raft_cli::parse_fragment_paf_min(copy, v);
    free(copy);
    return ok;
}

int main()
{
    using namespace raft_cli;
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
    CHECK(fragment_paf_options_ok(false, false) && fragment_paf_options_ok(true, false) && fragment_paf_options_ok(true, true));
    CHECK(!fragment_paf_options_ok(false, true));
    // ... and leaves the rules of the options before it alone
    CHECK(unitigs_options_ok(true, true) && !unitigs_options_ok(true, false) && best_options_ok(true, 0) && !best_options_ok(true, -1));
    CHECK(ends_options_ok(-1, false) && !ends_options_ok(-1, true));
    // the strand is tokenised for --overlap-ends or for the lift, fields 10 and 11 for the filter alone
    CHECK(!strand_wanted(-1, false) && strand_wanted(0, false) && strand_wanted(-1, true) && strand_wanted(1000, true));
    CHECK(paf_columns_with_lift(false, -1, false) == 0);
    CHECK(paf_columns_with_lift(false, -1, true) == RAFT_HOST_PAF_STRAND);
    CHECK(paf_columns_with_lift(false, 100, false) == RAFT_HOST_PAF_STRAND && paf_columns_with_lift(false, 100, true) == RAFT_HOST_PAF_STRAND);
    CHECK(paf_columns_with_lift(true, -1, false) == RAFT_HOST_PAF_QUALITY);
    CHECK(paf_columns_with_lift(true, -1, true) == (RAFT_HOST_PAF_QUALITY | RAFT_HOST_PAF_STRAND));
    CHECK(paf_columns_with_lift(true, 0, true) == (RAFT_HOST_PAF_QUALITY | RAFT_HOST_PAF_STRAND));
    for (int filter = 0; filter < 2; ++filter)
        for (int ends = -1; ends < 2; ++ends)                // without the option: the mask the job had
            CHECK(paf_columns_with_lift(filter != 0, ends, false) == paf_columns(filter != 0, ends >= 0));
    // the query ids are kept past prepare_input for the lift as for --fragment-overlaps
    CHECK(!keeps_query_ids_with_lift(false, 0, false, true) && !keeps_query_ids_with_lift(true, 0, false, false));
    CHECK(keeps_query_ids_with_lift(true, 0, false, true) && keeps_query_ids_with_lift(true, 0, true, false) && keeps_query_ids_with_lift(true, 1000, false, false));
    for (int prepare = 0; prepare < 2; ++prepare)
        for (int anchor = 0; anchor < 2; ++anchor)
            for (int frag = 0; frag < 2; ++frag)
                CHECK(keeps_query_ids_with_lift(prepare != 0, anchor, frag != 0, false) == keeps_query_ids(prepare != 0, anchor, frag != 0));
    // the stdout line
    CHECK(fragment_paf_line(1, 25236, 31002, 5112, 17, 3, 6) ==
          "INFO, fragment_paf(), min_len = 1, records = 25236, lifted = 31002, cut = 5112, without a fragment pair = 17, dropped pairs = 3, "
          "most from one record = 6");
    CHECK(fragment_paf_line(501, 0, 0, 0, 0, 0, 0) ==
          "INFO, fragment_paf(), min_len = 501, records = 0, lifted = 0, cut = 0, without a fragment pair = 0, dropped pairs = 0, most from one record = 0");
    CHECK(fragment_paf_line(2147483647, 1073741823, 2147483646, 1073741822, 1, 4611686018427387903LL, 1600) ==
          "INFO, fragment_paf(), min_len = 2147483647, records = 1073741823, lifted = 2147483646, cut = 1073741822, without a fragment pair = 1, "
          "dropped pairs = 4611686018427387903, most from one record = 1600");
    printf("cli_plan_lift_check: ok\n");
    return 0;
}
