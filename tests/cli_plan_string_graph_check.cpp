// cli_plan_string_graph_check.cpp -- what `raft --string-graph` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a program of its
// own (tests/test_cli_plan_string_graph.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

#include <set>
#include <string>

int main()
{
    using namespace raft_cli;
    // the two tables before stay what they were, long_option still counts through those two, and any_long_option through all three
    CHECK(sizeof kLongOptions / sizeof kLongOptions[0] == 13 && sizeof kLaterLongOptions / sizeof kLaterLongOptions[0] == 1);
    CHECK(sizeof kStringGraphLongOptions / sizeof kStringGraphLongOptions[0] == 2);
    CHECK(long_option_count() == 14 && any_long_option_count() == 16);
    for (size_t k = 0; k < 13; ++k) CHECK(&any_long_option(k) == &kLongOptions[k] && &long_option(k) == &kLongOptions[k], "row %zu", k);
    CHECK(&any_long_option(13) == &kLaterLongOptions[0] && &long_option(13) == &kLaterLongOptions[0]);
    CHECK(&any_long_option(14) == &kStringGraphLongOptions[0] && &any_long_option(15) == &kStringGraphLongOptions[1]);
    std::set<std::string> names;
    for (size_t k = 0; k < any_long_option_count(); ++k) names.insert(any_long_option(k).name);
    CHECK(names.size() == 16, "the names are unique over the three tables");
    {
        const LongOption &flag = any_long_option(14), &fuzz = any_long_option(15);
        CHECK(std::string(flag.name) == "string-graph" && flag.parse == nullptr && flag.value == nullptr && flag.flag == &Options::string_graph);
        CHECK(std::string(fuzz.name) == "string-graph-fuzz" && fuzz.parse == parse_string_graph_fuzz && fuzz.value == &Options::string_graph_fuzz &&
              fuzz.flag == &Options::string_graph_fuzz_given);
        const Options none;
        CHECK(!none.string_graph && !none.string_graph_fuzz_given && none.string_graph_fuzz == 1000 && kStringGraphFuzzDefault == 1000);
        Options got;
        CHECK(set_long_option(flag, nullptr, &got) && got.string_graph && !got.string_graph_fuzz_given && got.string_graph_fuzz == 1000);
        // ... and nothing else: every other value is what the command line leaves without it
        CHECK(got.overlap_ends == none.overlap_ends && got.ends_min_ratio == none.ends_min_ratio && !got.ends_ratio_given && !got.best_overlaps &&
              !got.unitigs && !got.components && !got.fragment_paf && !got.fragment_paf_min_given && !got.read_stats && !got.fragment_overlaps &&
              !got.repeat_stats && got.low_cov == none.low_cov && got.min_anchor == 0 && got.min_identity == 0 && got.min_overlap == 0 &&
              got.fragment_paf_min == none.fragment_paf_min);
        // the fuzz: digits alone, 0 .. INT32_MAX; anything else leaves the value and the mark alone
        Options z;
        CHECK(set_long_option(fuzz, "0", &z) && z.string_graph_fuzz == 0 && z.string_graph_fuzz_given && !z.string_graph);
        CHECK(set_long_option(fuzz, "2147483647", &z) && z.string_graph_fuzz == 2147483647);
        CHECK(set_long_option(fuzz, "0012", &z) && z.string_graph_fuzz == 12);
        for (const char *bad : {"", "-1", "+1", "1.5", "1e3", " 7", "7 ", "2147483648", "99999999999999999999", "x", "0x10"}) {
            Options b;
            CHECK(!set_long_option(fuzz, bad, &b) && b.string_graph_fuzz == 1000 && !b.string_graph_fuzz_given, "fuzz '%s'", bad);
        }
    }
    // usage_ok over every combination of the ten values its rules read, against the seven rules written out
    for (int c = 0; c < 512; ++c) {
        Options o;
        o.overlap_ends = (c & 1) ? 100 : -1; o.ends_ratio_given = (c & 2) != 0; o.best_overlaps = (c & 4) != 0; o.unitigs = (c & 8) != 0;
        o.fragment_paf = (c & 16) != 0; o.fragment_paf_min_given = (c & 32) != 0; o.components = (c & 64) != 0;
        o.string_graph = (c & 128) != 0; o.string_graph_fuzz_given = (c & 256) != 0;
        const bool ends_ok = o.overlap_ends >= 0 || !o.ends_ratio_given, best_ok = !o.best_overlaps || o.overlap_ends >= 0;
        const bool unitigs_ok = !o.unitigs || o.best_overlaps, lift_ok = o.fragment_paf || !o.fragment_paf_min_given;
        const bool components_ok = !o.components || o.overlap_ends >= 0;
        const bool graph_ok = !o.string_graph || o.overlap_ends >= 0, fuzz_ok = o.string_graph || !o.string_graph_fuzz_given;
        CHECK(usage_ok(o) == (ends_ok && best_ok && unitigs_ok && lift_ok && components_ok && graph_ok && fuzz_ok), "usage_ok, combination %d", c);
        for (int32_t z : {0, 2147483647}) {                // (the value itself has no say)
            Options v = o;
            v.string_graph_fuzz = z;
            CHECK(usage_ok(v) == usage_ok(o));
        }
    }
    {
        Options o;
        o.string_graph = true;
        CHECK(!usage_ok(o));
        o.overlap_ends = 0;                                // (H = 0 is an --overlap-ends)
        CHECK(usage_ok(o));
        o.string_graph_fuzz_given = true;
        CHECK(usage_ok(o));
        o.string_graph = false;
        CHECK(!usage_ok(o));
    }
    // the option asks nothing new of the job: the strand is --overlap-ends', and no query ids are kept for it
    for (int c = 0; c < 16; ++c) {
        Options with, without;
        with.overlap_ends = without.overlap_ends = (c & 1) ? 100 : -1;
        with.min_overlap = without.min_overlap = (c & 2) ? 500 : 0;
        with.fragment_paf = without.fragment_paf = (c & 8) != 0;
        with.string_graph = true; with.string_graph_fuzz = 7; with.string_graph_fuzz_given = true;
        const Request a = request(with, (c & 4) != 0), b = request(without, (c & 4) != 0);
        CHECK(a.filter == b.filter && a.strand == b.strand && a.quality_kept == b.quality_kept && a.paf_columns == b.paf_columns &&
              a.keep_query_ids == b.keep_query_ids && a.survey == b.survey && a.repeat_stats_second_pass == b.repeat_stats_second_pass, "request, combination %d", c);
    }
    // the edge list's first size: never 0, never more than two a record, about two a read
    CHECK(string_graph_capacity0(0, 0) == 1 && string_graph_capacity0(0, 2147483647) == 1 && string_graph_capacity0(1, 0) == 2);
    CHECK(string_graph_capacity0(5, 1000) == 10 && string_graph_capacity0(1000000, 300) == 1624);
    CHECK(string_graph_capacity0((int64_t(1) << 30) - 1, 1073741823) == 2147483646LL && string_graph_capacity0(int64_t(1) << 40, 1073741823) == 2147484670LL);
    // the stdout line
    CHECK(string_graph_line(1000, 25236, 9000, 120, 8800, 200, 0, 6100, 4400, 1350, 2500, 40, 95, 2380, 37, 11, 300) ==
          "INFO, string_graph(), fuzz = 1000, records = 25236, dovetail views = 9000, left out = 120, arcs = 8800, duplicates = 200, unpaired = 0, "
          "reducible = 6100, edges = 4400, kept = 1350, ends with one = 2500, ends that branch = 40, dead ends = 95, mutual ends = 2380, "
          "reads left out = 37 of 300, longest row = 11");
    CHECK(string_graph_line(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) ==
          "INFO, string_graph(), fuzz = 0, records = 0, dovetail views = 0, left out = 0, arcs = 0, duplicates = 0, unpaired = 0, reducible = 0, "
          "edges = 0, kept = 0, ends with one = 0, ends that branch = 0, dead ends = 0, mutual ends = 0, reads left out = 0 of 0, longest row = 0");
    const int64_t B = 9223372036854775807LL;
    CHECK(string_graph_line(2147483647, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B) ==
          "INFO, string_graph(), fuzz = 2147483647, records = 9223372036854775807, dovetail views = 9223372036854775807, left out = 9223372036854775807, "
          "arcs = 9223372036854775807, duplicates = 9223372036854775807, unpaired = 9223372036854775807, reducible = 9223372036854775807, "
          "edges = 9223372036854775807, kept = 9223372036854775807, ends with one = 9223372036854775807, ends that branch = 9223372036854775807, "
          "dead ends = 9223372036854775807, mutual ends = 9223372036854775807, reads left out = 9223372036854775807 of 9223372036854775807, "
          "longest row = 9223372036854775807");
    return cli_check::finish("cli_plan_string_graph_check");
}
