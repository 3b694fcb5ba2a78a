// cli_plan_graph_clean_check.cpp -- what `raft --graph-clean` adds to raft_amd/host/cli_plan.hpp, checked on the CPU as a program of its own
// (tests/test_cli_plan_graph_clean.py builds it under the address and undefined-behaviour sanitizers).
#include "cli_check.hpp"

#include <set>
#include <string>

int main()
{
    using namespace raft_cli;
    // the four new rows stand in the open table (whose length nothing here counts), under names no row of the closed tables has
    const LongOption *flag = nullptr, *ratio = nullptr, *tip = nullptr, *rounds = nullptr;
    std::set<std::string> names;
    for (size_t k = 0; k < every_long_option_count(); ++k) names.insert(every_long_option(k).name);
    const size_t closed = names.size();
    for (size_t k = 0; k < kOpenLongOptionCount; ++k) {
        const LongOption &o = kOpenLongOptions[k];
        names.insert(o.name);
        if (std::string(o.name) == "graph-clean") flag = &o;
        if (std::string(o.name) == "clean-min-ratio") ratio = &o;
        if (std::string(o.name) == "clean-tip-reads") tip = &o;
        if (std::string(o.name) == "clean-rounds") rounds = &o;
    }
    CHECK(names.size() == closed + kOpenLongOptionCount, "the names are unique over the closed tables and the open one");
    CHECK(flag && ratio && tip && rounds);
    CHECK(flag->parse == nullptr && flag->value == nullptr && flag->flag == &Options::graph_clean);
    CHECK(ratio->parse == parse_clean_min_ratio && ratio->value == &Options::clean_min_ratio && ratio->flag == &Options::clean_min_ratio_given);
    CHECK(tip->parse == parse_clean_tip_reads && tip->value == &Options::clean_tip_reads && tip->flag == &Options::clean_tip_reads_given);
    CHECK(rounds->parse == parse_clean_rounds && rounds->value == &Options::clean_rounds && rounds->flag == &Options::clean_rounds_given);
    const Options none;
    CHECK(!none.graph_clean && none.clean_min_ratio == 500 && none.clean_tip_reads == 4 && none.clean_rounds == 3);
    CHECK(!none.clean_min_ratio_given && !none.clean_tip_reads_given && !none.clean_rounds_given);
    CHECK(kCleanMinRatioDefault == 500 && kCleanTipReadsDefault == 4 && kCleanRoundsDefault == 3 && kCleanRoundsMax == 64);
    {
        Options got;
        CHECK(set_long_option(*flag, nullptr, &got) && got.graph_clean && !got.clean_min_ratio_given && !got.clean_tip_reads_given && !got.clean_rounds_given);
        // ... and nothing else: every other value is what the command line leaves without it
        CHECK(got.overlap_ends == none.overlap_ends && !got.best_overlaps && !got.unitigs && !got.components && !got.string_graph && !got.containment &&
              !got.string_graph_fuzz_given && !got.fragment_paf && !got.read_stats && got.clean_min_ratio == 500 && got.clean_tip_reads == 4 &&
              got.clean_rounds == 3);
    }
    // the parsers at their bounds: digits alone; anything else leaves the value and the mark alone
    {
        Options z;
        CHECK(set_long_option(*ratio, "0", &z) && z.clean_min_ratio == 0 && z.clean_min_ratio_given && !z.graph_clean);
        CHECK(set_long_option(*ratio, "1000", &z) && z.clean_min_ratio == 1000);
        CHECK(set_long_option(*ratio, "0500", &z) && z.clean_min_ratio == 500);
        CHECK(set_long_option(*tip, "0", &z) && z.clean_tip_reads == 0 && z.clean_tip_reads_given);
        CHECK(set_long_option(*tip, "2147483647", &z) && z.clean_tip_reads == 2147483647);
        CHECK(set_long_option(*rounds, "1", &z) && z.clean_rounds == 1 && z.clean_rounds_given);
        CHECK(set_long_option(*rounds, "64", &z) && z.clean_rounds == 64);
        CHECK(set_long_option(*rounds, "007", &z) && z.clean_rounds == 7);
        for (const char *bad : {"", "-1", "+1", "1.5", "1e2", " 7", "7 ", "1001", "2147483648", "99999999999999999999", "x"}) {
            Options b;
            CHECK(!set_long_option(*ratio, bad, &b) && b.clean_min_ratio == 500 && !b.clean_min_ratio_given, "ratio '%s'", bad);
        }
        for (const char *bad : {"", "-1", "+1", "1.5", " 7", "2147483648", "99999999999999999999", "x", "0x10"}) {
            Options b;
            CHECK(!set_long_option(*tip, bad, &b) && b.clean_tip_reads == 4 && !b.clean_tip_reads_given, "tip reads '%s'", bad);
        }
        for (const char *bad : {"", "0", "00", "65", "-1", "+1", "1.5", " 7", "2147483648", "99999999999999999999", "x"}) {
            Options b;
            CHECK(!set_long_option(*rounds, bad, &b) && b.clean_rounds == 3 && !b.clean_rounds_given, "rounds '%s'", bad);
        }
    }
    // usage_ok: --graph-clean needs --string-graph (which needs --overlap-ends); each valued option needs --graph-clean
    for (int c = 0; c < 64; ++c) {
        Options o;
        o.overlap_ends = (c & 1) ? 100 : -1; o.string_graph = (c & 2) != 0; o.graph_clean = (c & 4) != 0;
        o.clean_min_ratio_given = (c & 8) != 0; o.clean_tip_reads_given = (c & 16) != 0; o.clean_rounds_given = (c & 32) != 0;
        const bool graph_ok = !o.string_graph || o.overlap_ends >= 0, clean_ok = !o.graph_clean || o.string_graph;
        const bool values_ok = o.graph_clean || !(o.clean_min_ratio_given || o.clean_tip_reads_given || o.clean_rounds_given);
        CHECK(usage_ok(o) == (graph_ok && clean_ok && values_ok), "usage_ok, combination %d", c);
    }
    {
        Options o;
        o.graph_clean = true;
        CHECK(!usage_ok(o));
        o.overlap_ends = 0;
        CHECK(!usage_ok(o));                               // (--overlap-ends alone is not --string-graph)
        o.string_graph = true;
        CHECK(usage_ok(o));
        o.clean_rounds_given = o.clean_tip_reads_given = o.clean_min_ratio_given = true;
        CHECK(usage_ok(o));
    }
    // the option asks nothing new of the job
    for (int c = 0; c < 8; ++c) {
        Options with, without;
        with.overlap_ends = without.overlap_ends = 100;
        with.string_graph = without.string_graph = true;
        with.min_overlap = without.min_overlap = (c & 1) ? 500 : 0;
        with.fragment_paf = without.fragment_paf = (c & 2) != 0;
        with.graph_clean = true;
        const Request a = request(with, (c & 4) != 0), b = request(without, (c & 4) != 0);
        CHECK(a.filter == b.filter && a.strand == b.strand && a.quality_kept == b.quality_kept && a.paf_columns == b.paf_columns &&
              a.keep_query_ids == b.keep_query_ids && a.survey == b.survey && a.repeat_stats_second_pass == b.repeat_stats_second_pass, "request, combination %d", c);
    }
    // the two stdout lines
    CHECK(graph_clean_line(500, 4, 2, 3, 1, 9000, 120, 31, 40, 250000, 44, 8836, 17, 9, 5) ==
          "INFO, graph_clean(), min_ratio = 500 per mille, tip_reads = 4, rounds = 2 of 3, converged = 1, edges = 9000, weak edges = 120, tips = 31, "
          "tip reads = 40, tip bases = 250000, tip edges = 44, kept edges = 8836, ends that branch = 17, dead ends = 9, short isolated chains = 5");
    CHECK(graph_clean_line(0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) ==
          "INFO, graph_clean(), min_ratio = 0 per mille, tip_reads = 0, rounds = 1 of 1, converged = 1, edges = 0, weak edges = 0, tips = 0, tip reads = 0, "
          "tip bases = 0, tip edges = 0, kept edges = 0, ends that branch = 0, dead ends = 0, short isolated chains = 0");
    const int64_t B = 9223372036854775807LL;
    CHECK(graph_clean_line(1000, 2147483647, B, 64, B, B, B, B, B, B, B, B, B, B, B) ==
          "INFO, graph_clean(), min_ratio = 1000 per mille, tip_reads = 2147483647, rounds = 9223372036854775807 of 64, converged = 9223372036854775807, "
          "edges = 9223372036854775807, weak edges = 9223372036854775807, tips = 9223372036854775807, tip reads = 9223372036854775807, "
          "tip bases = 9223372036854775807, tip edges = 9223372036854775807, kept edges = 9223372036854775807, ends that branch = 9223372036854775807, "
          "dead ends = 9223372036854775807, short isolated chains = 9223372036854775807");
    CHECK(graph_clean_unitigs_line(5000, 120, 40, 7, 1, 900, 8000000, 9000000, 4000000) ==
          "INFO, graph_clean_unitigs(), reads = 5000, left out = 120, unitigs = 40, singletons = 7, circular = 1, longest = 900 reads, "
          "longest length = 8000000, total length = 9000000, N50 = 4000000");
    // ... with the fields of unitigs_line, whatever they are
    CHECK(graph_clean_unitigs_line(1, 2, 3, 4, 5, 6, 7, 8, 9) == "INFO, graph_clean_unitigs()" + unitigs_line(1, 2, 3, 4, 5, 6, 7, 8, 9).substr(15));
    CHECK(unitigs_line(1, 2, 3, 4, 5, 6, 7, 8, 9).substr(0, 15) == "INFO, unitigs()");
    return cli_check::finish("cli_plan_graph_clean_check");
}
