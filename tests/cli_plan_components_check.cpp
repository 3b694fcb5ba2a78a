// cli_plan_components_check.cpp -- what `raft --components` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a program of its
// own (tests/test_cli_plan_components.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

#include <set>
#include <string>

int main()
{
    using namespace raft_cli;
    // the thirteen stay, the new row stands behind them, and long_option counts through both
    CHECK(sizeof kLongOptions / sizeof kLongOptions[0] == 13 && sizeof kLaterLongOptions / sizeof kLaterLongOptions[0] == 1);
    CHECK(long_option_count() == 14);
    for (size_t k = 0; k < 13; ++k) CHECK(&long_option(k) == &kLongOptions[k], "row %zu", k);
    CHECK(&long_option(13) == &kLaterLongOptions[0]);
    std::set<std::string> names;
    for (size_t k = 0; k < long_option_count(); ++k) names.insert(long_option(k).name);
    CHECK(names.size() == 14, "the names are unique over both tables");
    {
        const LongOption &o = long_option(13);
        CHECK(std::string(o.name) == "components" && o.parse == nullptr && o.value == nullptr && o.flag == &Options::components);
        Options got;
        CHECK(!got.components);
        CHECK(set_long_option(o, nullptr, &got) && got.components);
        // ... and nothing else: every other value is what the command line leaves without it
        const Options none;
        CHECK(got.overlap_ends == none.overlap_ends && got.ends_min_ratio == none.ends_min_ratio && !got.ends_ratio_given && !got.best_overlaps &&
              !got.unitigs && !got.fragment_paf && !got.fragment_paf_min_given && !got.read_stats && !got.fragment_overlaps && !got.repeat_stats &&
              got.low_cov == none.low_cov && got.min_anchor == 0 && got.min_identity == 0 && got.min_overlap == 0 && got.fragment_paf_min == none.fragment_paf_min);
    }
    // usage_ok over every combination of the seven values its rules read, against the five rules written out
    for (int c = 0; c < 128; ++c) {
        Options o;
        o.overlap_ends = (c & 1) ? 100 : -1; o.ends_ratio_given = (c & 2) != 0; o.best_overlaps = (c & 4) != 0; o.unitigs = (c & 8) != 0;
        o.fragment_paf = (c & 16) != 0; o.fragment_paf_min_given = (c & 32) != 0; o.components = (c & 64) != 0;
        const bool ends_ok = o.overlap_ends >= 0 || !o.ends_ratio_given, best_ok = !o.best_overlaps || o.overlap_ends >= 0;
        const bool unitigs_ok = !o.unitigs || o.best_overlaps, lift_ok = o.fragment_paf || !o.fragment_paf_min_given;
        const bool components_ok = !o.components || o.overlap_ends >= 0;
        CHECK(usage_ok(o) == (ends_ok && best_ok && unitigs_ok && lift_ok && components_ok), "usage_ok, combination %d", c);
    }
    {
        Options o;
        o.components = true;
        CHECK(!usage_ok(o));
        o.overlap_ends = 0;                                // (H = 0 is an --overlap-ends)
        CHECK(usage_ok(o));
    }
    // the option asks nothing new of the job: the strand is --overlap-ends', and no query ids are kept for it
    for (int c = 0; c < 8; ++c) {
        Options with, without;
        with.overlap_ends = without.overlap_ends = (c & 1) ? 100 : -1;
        with.min_overlap = without.min_overlap = (c & 2) ? 500 : 0;
        with.components = true;
        const Request a = request(with, (c & 4) != 0), b = request(without, (c & 4) != 0);
        CHECK(a.filter == b.filter && a.strand == b.strand && a.quality_kept == b.quality_kept && a.paf_columns == b.paf_columns &&
              a.keep_query_ids == b.keep_query_ids && a.survey == b.survey && a.repeat_stats_second_pass == b.repeat_stats_second_pass, "request, combination %d", c);
    }
    // the stdout line
    CHECK(components_line(60, 25236, 20118, 57, 31, 211, 2310045, 3301922, 703, 300) ==
          "INFO, components(), kinds = 60, records = 25236, edges = 20118, components = 57, singletons = 31, largest = 211 reads, "
          "largest bases = 2310045 of 3301922, reads in the largest = 703 per mille of 300");
    CHECK(components_line(62, 0, 0, 0, 0, 0, 0, 0, 0, 0) ==
          "INFO, components(), kinds = 62, records = 0, edges = 0, components = 0, singletons = 0, largest = 0 reads, largest bases = 0 of 0, "
          "reads in the largest = 0 per mille of 0");
    CHECK(components_line(2, 4611686018427387903LL, 4611686018427387902LL, 2147483647, 2147483646, 2147483647, 2305843009213693951LL,
                          4611686018427387903LL, 1000, 2147483647) ==
          "INFO, components(), kinds = 2, records = 4611686018427387903, edges = 4611686018427387902, components = 2147483647, "
          "singletons = 2147483646, largest = 2147483647 reads, largest bases = 2305843009213693951 of 4611686018427387903, "
          "reads in the largest = 1000 per mille of 2147483647");
    return cli_check::finish("cli_plan_components_check");
}
