// cli_plan_containment_check.cpp -- what `raft --containment` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a program of its own
// (tests/test_cli_plan_containment.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

#include <set>
#include <string>

int main()
{
    using namespace raft_cli;
    // the three tables before stay what they were, and so do the two accessors over them
    CHECK(sizeof kLongOptions / sizeof kLongOptions[0] == 13 && sizeof kLaterLongOptions / sizeof kLaterLongOptions[0] == 1);
    CHECK(sizeof kStringGraphLongOptions / sizeof kStringGraphLongOptions[0] == 2 && sizeof kContainmentLongOptions / sizeof kContainmentLongOptions[0] == 1);
    CHECK(long_option_count() == 14 && any_long_option_count() == 16 && every_long_option_count() == 17);
    for (size_t k = 0; k < 13; ++k) CHECK(&any_long_option(k) == &kLongOptions[k] && &long_option(k) == &kLongOptions[k], "row %zu", k);
    CHECK(&any_long_option(13) == &kLaterLongOptions[0] && &long_option(13) == &kLaterLongOptions[0]);
    CHECK(&any_long_option(14) == &kStringGraphLongOptions[0] && &any_long_option(15) == &kStringGraphLongOptions[1]);
    // one list of tables, walked end to end: the sixteen as any_long_option has them, then the new row
    CHECK(sizeof kLongOptionTables / sizeof kLongOptionTables[0] == 4);
    CHECK(kLongOptionTables[0].rows == kLongOptions && kLongOptionTables[1].rows == kLaterLongOptions && kLongOptionTables[2].rows == kStringGraphLongOptions &&
          kLongOptionTables[3].rows == kContainmentLongOptions);
    CHECK(kLongOptionTables[0].count == 13 && kLongOptionTables[1].count == 1 && kLongOptionTables[2].count == 2 && kLongOptionTables[3].count == 1);
    for (size_t k = 0; k < 16; ++k) CHECK(&every_long_option(k) == &any_long_option(k), "row %zu", k);
    CHECK(&every_long_option(16) == &kContainmentLongOptions[0]);
    std::set<std::string> names;
    for (size_t k = 0; k < every_long_option_count(); ++k) names.insert(every_long_option(k).name);
    CHECK(names.size() == 17, "the names are unique over the four tables");
    {
        const LongOption &flag = every_long_option(16);
        CHECK(std::string(flag.name) == "containment" && flag.parse == nullptr && flag.value == nullptr && flag.flag == &Options::containment);
        const Options none;
        CHECK(!none.containment);
        Options got;
        CHECK(set_long_option(flag, nullptr, &got) && got.containment);
        // ... and nothing else: every other value is what the command line leaves without it
        CHECK(got.overlap_ends == none.overlap_ends && got.ends_min_ratio == none.ends_min_ratio && !got.ends_ratio_given && !got.best_overlaps &&
              !got.unitigs && !got.components && !got.string_graph && !got.string_graph_fuzz_given && got.string_graph_fuzz == none.string_graph_fuzz &&
              !got.fragment_paf && !got.fragment_paf_min_given && !got.read_stats && !got.fragment_overlaps && !got.repeat_stats &&
              got.low_cov == none.low_cov && got.min_anchor == 0 && got.min_identity == 0 && got.min_overlap == 0 && got.fragment_paf_min == none.fragment_paf_min);
    }
    // usage_ok over every combination of the values its rules read, against the eight rules written out
    for (int c = 0; c < 1024; ++c) {
        Options o;
        o.overlap_ends = (c & 1) ? 100 : -1; o.ends_ratio_given = (c & 2) != 0; o.best_overlaps = (c & 4) != 0; o.unitigs = (c & 8) != 0;
        o.fragment_paf = (c & 16) != 0; o.fragment_paf_min_given = (c & 32) != 0; o.components = (c & 64) != 0;
        o.string_graph = (c & 128) != 0; o.string_graph_fuzz_given = (c & 256) != 0; o.containment = (c & 512) != 0;
        const bool ends_ok = o.overlap_ends >= 0 || !o.ends_ratio_given, best_ok = !o.best_overlaps || o.overlap_ends >= 0;
        const bool unitigs_ok = !o.unitigs || o.best_overlaps, lift_ok = o.fragment_paf || !o.fragment_paf_min_given;
        const bool components_ok = !o.components || o.overlap_ends >= 0;
        const bool graph_ok = !o.string_graph || o.overlap_ends >= 0, fuzz_ok = o.string_graph || !o.string_graph_fuzz_given;
        const bool containment_ok = !o.containment || o.overlap_ends >= 0;
        CHECK(usage_ok(o) == (ends_ok && best_ok && unitigs_ok && lift_ok && components_ok && graph_ok && fuzz_ok && containment_ok), "usage_ok, combination %d", c);
    }
    {
        Options o;
        o.containment = true;
        CHECK(!usage_ok(o));
        o.overlap_ends = 0;                                // (H = 0 is an --overlap-ends)
        CHECK(usage_ok(o));
        o.unitigs = true;                                  // (--unitigs still needs --best-overlaps, with or without the option)
        CHECK(!usage_ok(o));
        o.best_overlaps = true;
        CHECK(usage_ok(o));
    }
    // the option asks nothing new of the job: the strand is --overlap-ends', and no query ids are kept for it
    for (int c = 0; c < 16; ++c) {
        Options with, without;
        with.overlap_ends = without.overlap_ends = (c & 1) ? 100 : -1;
        with.min_overlap = without.min_overlap = (c & 2) ? 500 : 0;
        with.fragment_paf = without.fragment_paf = (c & 8) != 0;
        with.containment = true;
        const Request a = request(with, (c & 4) != 0), b = request(without, (c & 4) != 0);
        CHECK(a.filter == b.filter && a.strand == b.strand && a.quality_kept == b.quality_kept && a.paf_columns == b.paf_columns &&
              a.keep_query_ids == b.keep_query_ids && a.survey == b.survey && a.repeat_stats_second_pass == b.repeat_stats_second_pass, "request, combination %d", c);
    }
    // the two stdout lines
    CHECK(containment_line(25236, 9000, 12, 4100, 3, 900, 410, 5, 77, 1234567) ==
          "INFO, containment(), records = 25236, containment views = 9000, not longer = 12, reads with a parent = 4100, contained without a parent = 3, "
          "roots = 900, roots with a tree = 410, deepest = 5, largest tree = 77 reads, largest tree bases = 1234567");
    CHECK(containment_line(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) ==
          "INFO, containment(), records = 0, containment views = 0, not longer = 0, reads with a parent = 0, contained without a parent = 0, roots = 0, "
          "roots with a tree = 0, deepest = 0, largest tree = 0 reads, largest tree bases = 0");
    const int64_t B = 9223372036854775807LL;
    CHECK(containment_line(B, B, B, B, B, B, B, B, B, B) ==
          "INFO, containment(), records = 9223372036854775807, containment views = 9223372036854775807, not longer = 9223372036854775807, "
          "reads with a parent = 9223372036854775807, contained without a parent = 9223372036854775807, roots = 9223372036854775807, "
          "roots with a tree = 9223372036854775807, deepest = 9223372036854775807, largest tree = 9223372036854775807 reads, "
          "largest tree bases = 9223372036854775807");
    CHECK(place_contained_line(40, 4900, 100, 5000, 31, 17250) ==
          "INFO, place_contained(), unitigs = 40, placed = 4900, unplaced = 100 of 5000, unitigs that gained reads = 31, greatest depth = 17250 per mille");
    CHECK(place_contained_line(0, 0, 0, 0, 0, 0) ==
          "INFO, place_contained(), unitigs = 0, placed = 0, unplaced = 0 of 0, unitigs that gained reads = 0, greatest depth = 0 per mille");
    CHECK(place_contained_line(B, B, B, B, B, B) ==
          "INFO, place_contained(), unitigs = 9223372036854775807, placed = 9223372036854775807, unplaced = 9223372036854775807 of 9223372036854775807, "
          "unitigs that gained reads = 9223372036854775807, greatest depth = 9223372036854775807 per mille");
    return cli_check::finish("cli_plan_containment_check");
}
