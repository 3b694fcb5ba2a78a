// cli_plan_check.cpp -- raft_amd/host/cli_plan.hpp on its own: the device list, the output capacities, the record estimate, the
// sampled run count, the coverage widths, the ladder after an overflowing exception list, the start-time field and the two
// descriptions of the stage clock; the table of the long options and what the options ask of a job between them (Request).  No HIP:
// a host compiler builds it (tests/test_cli_plan.py: under the address and undefined-behaviour sanitizers).  Every expected value
// is a literal: what the statements of the former main() (raft_main.cpp at 451f851, lines 139-181, 238-267, 425-437, 469-479) gave
// on the same inputs; for the Request, the expressions of the functions it replaced, written out.
#include "cli_check.hpp"

#include <initializer_list>
#include <set>

using namespace raft_cli;

static const char *show(const char *s) { return s ? s : "(unset)"; }

static void dev(const char *devices, const char *device, const char *ranks_text, int ranks, std::initializer_list<int> ids)
{
    const DeviceList l = device_list(devices, device, ranks_text);
    CHECK(l.ranks == ranks, "RAFT_DEVICES=%s RAFT_DEVICE=%s RAFT_RANKS=%s: ranks %d, want %d", show(devices), show(device), show(ranks_text), l.ranks, ranks);
    CHECK(l.devices == std::vector<int>(ids), "RAFT_DEVICES=%s RAFT_DEVICE=%s RAFT_RANKS=%s: %zu devices, first %d", show(devices), show(device), show(ranks_text),
          l.devices.size(), l.devices.empty() ? -1 : l.devices[0]);
}

static void caps(std::vector<int32_t> len, int reso, int repeat_length, int interval_length, long long n_win, long long rep_cap, long long frag_cap,
                 long long exc_cap0, long long n_anchor, long long cov8_bytes)
{
    const Capacities c = output_capacities((int32_t)len.size(), len.data(), reso, repeat_length, interval_length);
    CHECK(c.n_win == n_win && c.rep_cap == rep_cap && c.frag_cap == frag_cap && c.exc_cap0 == exc_cap0 && c.n_anchor == n_anchor && c.cov8_bytes == cov8_bytes,
          "%zu reads, reso %d, repeat_length %d, interval_length %d: %lld %lld %lld %lld %lld %lld", len.size(), reso, repeat_length, interval_length, (long long)c.n_win,
          (long long)c.rep_cap, (long long)c.frag_cap, (long long)c.exc_cap0, (long long)c.n_anchor, (long long)c.cov8_bytes);
}

static void est(long long size, const char *name, long long want)
{
    CHECK(record_estimate(size, name) == want, "%lld bytes of %s: %lld, want %lld", size, name, (long long)record_estimate(size, name), want);
}

// An ascending query column of n_rec records with single low values in it: "sampledN" puts N of them on sampled positions,
// "betweenN" one record behind a sampled position (which is a sampled position itself where every record is sampled).
static std::vector<int32_t> make_q(const char *kind, int64_t n_rec)
{
    std::vector<int32_t> q((size_t)n_rec);
    for (int64_t i = 0; i < n_rec; ++i) q[(size_t)i] = (int32_t)i;
    const int64_t S = std::min<int64_t>(n_rec, 8192);
    auto pos = [&](int64_t i) { return S > 1 ? i * (n_rec - 1) / (S - 1) : 0; };
    int n = 0;
    bool between = false;
    if (sscanf(kind, "sampled%d", &n) == 1) between = false;
    else if (sscanf(kind, "between%d", &n) == 1) between = true;
    else if (strcmp(kind, "descending") == 0) { for (int64_t i = 0; i < n_rec; ++i) q[(size_t)i] = (int32_t)(n_rec - i); return q; }
    for (int k = 1; k <= n; ++k) {               // n single low values, spread over the stream
        const int64_t i = std::max<int64_t>(1, (S - 1) * k / (n + 1));
        const int64_t at = pos(i) + (between ? 1 : 0);
        if (at < n_rec) q[(size_t)at] = -1;
    }
    return q;
}

// descents: those of the whole column, a check of the generator (what the samples see of them is `want`)
static void few(const char *kind, long long n_rec, int descents, bool want)
{
    const std::vector<int32_t> q = make_q(kind, n_rec);
    int all = 0;
    for (int64_t i = 1; i < n_rec; ++i) all += q[(size_t)i] < q[(size_t)i - 1];
    CHECK(all == descents, "%s, %lld records: the column has %d descents, not %d", kind, n_rec, all, descents);
    CHECK(few_sorted_runs(q.data(), n_rec) == want, "%s, %lld records: want %d", kind, n_rec, (int)want);
}

static void step(int cov_width, long long exc_cap, long long n_exc, long long n_win, int next_width, long long next_cap)
{
    const Attempt a = next_attempt(cov_width, exc_cap, n_exc, n_win);
    CHECK(a.cov_width == next_width && a.exc_cap == next_cap, "width %d, room %lld, %lld exceptions, %lld windows: width %d, room %lld", cov_width, exc_cap, n_exc, n_win,
          a.cov_width, (long long)a.exc_cap);
}

// every value of an Options, as text: two are equal when these are
static std::string fields(const Options &o)
{
    std::string t = o.prefix + " " + std::to_string(o.cov_mul);
    for (long long v : {(long long)o.reso, (long long)o.est_cov, (long long)o.repeat_length, (long long)o.interval_length, (long long)o.read_length,
                        (long long)o.overlap_length, (long long)o.flanking_length, (long long)o.auto_cov, (long long)o.read_stats, (long long)o.low_cov,
                        (long long)o.min_anchor, (long long)o.fragment_overlaps, (long long)o.repeat_stats, (long long)o.min_identity, (long long)o.min_overlap,
                        (long long)o.overlap_ends, (long long)o.ends_min_ratio, (long long)o.ends_ratio_given, (long long)o.best_overlaps, (long long)o.unitigs,
                        (long long)o.fragment_paf, (long long)o.fragment_paf_min, (long long)o.fragment_paf_min_given})
        t += " " + std::to_string(v);
    return t;
}

// One row of kLongOptions against what the former `case` of parse_options did: a flag sets `flag` and nothing else; a value option
// takes `good` -- a text that the other parsers of the table refuse or read differently -- into `value` (and sets `given`, where it
// has one), refuses `bad`, and a refused text changes nothing at all.
static void row(int k, const char *name, bool Options::*flag, int32_t Options::*value, const char *good, int32_t want, const char *bad)
{
    const LongOption &o = kLongOptions[k];
    CHECK(strcmp(o.name, name) == 0, "row %d is %s, want %s", k, o.name, name);
    CHECK((o.parse != nullptr) == (value != nullptr) && (o.value != nullptr) == (value != nullptr), "--%s: takes an argument exactly when it has a value", name);
    Options expect, got;
    if (value) expect.*value = want;
    if (flag) expect.*flag = true;
    char *text = good ? strdup(good) : nullptr;            // (a heap block of exactly the text's size)
    CHECK(set_long_option(o, text, &got) && fields(got) == fields(expect), "--%s %s: %s", name, good ? good : "", fields(got).c_str());
    free(text);
    if (bad) {
        Options untouched;
        text = strdup(bad);
        CHECK(!set_long_option(o, text, &untouched) && fields(untouched) == fields(Options()), "--%s %s is refused and changes nothing", name, bad);
        free(text);
    }
}

static void long_options()
{
    CHECK(sizeof kLongOptions / sizeof kLongOptions[0] == 13, "thirteen long options");
    std::set<std::string> names;
    for (const LongOption &o : kLongOptions) names.insert(o.name);
    CHECK(names.size() == 13, "the names are unique");
    row(0, "read-stats", &Options::read_stats, nullptr, nullptr, 0, nullptr);
    row(1, "low-cov", nullptr, &Options::low_cov, "0", 0, "-1");                         // (0: parse_low_cov takes it, parse_min_anchor does not)
    row(2, "repeat-overlaps", nullptr, &Options::min_anchor, "5", 5, "0");
    row(3, "fragment-overlaps", &Options::fragment_overlaps, nullptr, nullptr, 0, nullptr);
    row(4, "repeat-stats", &Options::repeat_stats, nullptr, nullptr, 0, nullptr);
    row(5, "min-identity", nullptr, &Options::min_identity, "99.5", 995, "100.1");       // (per mille: no other parser reads a point)
    row(6, "min-overlap", nullptr, &Options::min_overlap, "500", 500, "0");
    row(7, "overlap-ends", nullptr, &Options::overlap_ends, "1001", 1001, "2147483648");  // (1001: beyond parse_ends_min_ratio)
    row(8, "ends-min-ratio", &Options::ends_ratio_given, &Options::ends_min_ratio, "1000", 1000, "1001");
    row(9, "best-overlaps", &Options::best_overlaps, nullptr, nullptr, 0, nullptr);
    row(10, "unitigs", &Options::unitigs, nullptr, nullptr, 0, nullptr);
    row(11, "fragment-paf", &Options::fragment_paf, nullptr, nullptr, 0, nullptr);
    row(12, "fragment-paf-min", &Options::fragment_paf_min_given, &Options::fragment_paf_min, "501", 501, "0");
    row(7, "overlap-ends", nullptr, &Options::overlap_ends, "0", 0, "x");                 // (0: parse_overlap_ends takes it, parse_min_anchor does not)
    // what the command line leaves without any of them
    const Options none;
    CHECK(none.low_cov == -1 && none.overlap_ends == -1 && none.min_anchor == 0 && none.min_identity == 0 && none.min_overlap == 0 &&
          none.ends_min_ratio == kEndsMinRatioDefault && none.fragment_paf_min == kFragmentPafMinDefault && usage_ok(none), "the defaults");
    CHECK(none.reso == 50 && none.est_cov == 0 && none.cov_mul == 1.5 && none.repeat_length == 10000 && none.interval_length == 10000 &&
          none.read_length == 20000 && none.overlap_length == 500 && none.flanking_length == 1000 && none.prefix == "raft" && !none.auto_cov, "param.hpp:18-31");
}

// usage_ok over every combination of the six values its rules read, against the four rules it took over from the functions before it, written out
static void usage_rules()
{
    for (int c = 0; c < 64; ++c) {
        Options o;
        o.overlap_ends = (c & 1) ? 100 : -1; o.ends_ratio_given = (c & 2) != 0; o.best_overlaps = (c & 4) != 0; o.unitigs = (c & 8) != 0;
        o.fragment_paf = (c & 16) != 0; o.fragment_paf_min_given = (c & 32) != 0;
        const bool ends_ok = o.overlap_ends >= 0 || !o.ends_ratio_given, best_ok = !o.best_overlaps || o.overlap_ends >= 0;
        const bool unitigs_ok = !o.unitigs || o.best_overlaps, lift_ok = o.fragment_paf || !o.fragment_paf_min_given;
        CHECK(usage_ok(o) == (ends_ok && best_ok && unitigs_ok && lift_ok), "usage_ok, combination %d", c);
    }
}

// Every Request field over prepare, -e auto, the filter (either option, both, none), --overlap-ends and the eight other options,
// against the expressions of the eight functions it replaced (DESIGN.md I.21 names them) as they stood, written out over the same
// values.
static void requests()
{
    for (int c = 0; c < (1 << 13); ++c) {
        const bool prepare = c & 1;
        Options o;
        o.auto_cov = (c & 2) != 0; o.est_cov = o.auto_cov ? 0 : 30;
        o.min_identity = (c & 4) ? 990 : 0; o.min_overlap = (c & 8) ? 500 : 0;
        o.overlap_ends = (c & 16) ? 0 : -1;
        o.read_stats = (c & 32) != 0; o.low_cov = (c & 64) ? 0 : -1; o.min_anchor = (c & 128) ? 1 : 0; o.fragment_overlaps = (c & 256) != 0;
        o.repeat_stats = (c & 512) != 0; o.best_overlaps = (c & 1024) != 0; o.unitigs = (c & 2048) != 0; o.fragment_paf = (c & 4096) != 0;
        const Request r = request(o, prepare);
        const bool filter = o.min_identity > 0 || o.min_overlap > 0;
        const bool strand = o.overlap_ends >= 0 || o.fragment_paf;
        CHECK(r.filter == filter, "filter, combination %d", c);
        CHECK(r.strand == strand, "strand, combination %d", c);
        CHECK(r.quality_kept == (filter && o.fragment_paf), "quality_kept, combination %d", c);
        CHECK(r.paf_columns == ((filter ? RAFT_HOST_PAF_QUALITY : 0) | (strand ? RAFT_HOST_PAF_STRAND : 0)), "paf_columns, combination %d", c);
        CHECK(r.keep_query_ids == (prepare && (o.min_anchor > 0 || (o.fragment_overlaps || o.fragment_paf))), "keep_query_ids, combination %d", c);
        CHECK(r.survey == (o.auto_cov || o.read_stats || o.low_cov >= 0 || o.repeat_stats), "survey, combination %d", c);
        CHECK(r.repeat_stats_second_pass == (o.auto_cov && o.repeat_stats), "repeat_stats_second_pass, combination %d", c);
    }
}

int main()
{
    long_options();
    usage_rules();
    requests();
    // devices
    dev("0,1", nullptr, nullptr, 0, {0, 1});
    dev("0,1", "5", nullptr, 0, {0, 1});
    dev("0,0,0", nullptr, nullptr, 0, {0, 0, 0});
    dev("0,0,0", "5", nullptr, 0, {0, 0, 0});
    dev("3", nullptr, nullptr, 0, {3});
    dev("3", "5", nullptr, 0, {3});
    dev("", nullptr, nullptr, 0, {0});
    dev("", "5", nullptr, 0, {5});
    dev("1,x", nullptr, nullptr, 0, {1});
    dev("1,x", "5", nullptr, 0, {1});
    dev("2,,3", nullptr, nullptr, 0, {2});
    dev("2,,3", "5", nullptr, 0, {2});
    dev("0,7,", nullptr, nullptr, 0, {0, 7});
    dev("0,7,", "5", nullptr, 0, {0, 7});
    dev(" 4", nullptr, nullptr, 0, {4});
    dev(" 4", "5", nullptr, 0, {4});
    dev(nullptr, nullptr, nullptr, 0, {0});
    dev(nullptr, "5", nullptr, 0, {5});
    dev("0,1", nullptr, "0", 1, {0});
    dev(nullptr, "5", "0", 1, {5});
    dev("0,1", nullptr, "3", 3, {0, 1, 0});
    dev(nullptr, "5", "3", 3, {5, 5, 5});
    dev("0,1", nullptr, "100", 64, {0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1});
    dev(nullptr, "5", "100", 64, {5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5});
    dev("0,1", nullptr, "-2", 1, {0});
    dev(nullptr, "5", "-2", 1, {5});
    dev("2,,3", "6", "3", 3, {2, 2, 2});
    dev("0,7,", nullptr, "5", 5, {0, 7, 0, 7, 0});
    dev("", nullptr, "2", 2, {0, 0});
    dev("0,1", nullptr, "x", 1, {0});
    dev(nullptr, "x", nullptr, 0, {0});
    // capacities
    caps({}, 50, 10000, 10000, 0LL, 0LL, 0LL, 65536LL, 2LL, 2LL);
    caps({0, 1, 49, 50, 51}, 50, 10000, 10000, 5LL, 0LL, 10LL, 65536LL, 2LL, 12LL);
    caps({0, 1, 49, 50, 51}, 50, 100, 60, 5LL, 3LL, 12LL, 65536LL, 2LL, 12LL);
    caps({0, 1, 2, 3}, 1, 10000, 10000, 6LL, 0LL, 8LL, 65536LL, 2LL, 14LL);
    caps({0, 1, 2, 70000}, 1, 1, 1, 70003LL, 35003LL, 70011LL, 65536LL, 70LL, 140008LL);
    caps({20000, 30000, 12345}, 50, 49, 10000, 1247LL, 625LL, 12LL, 65536LL, 3LL, 2496LL);
    caps({20000, 30000, 12345}, 50, 1, 10000, 1247LL, 625LL, 12LL, 65536LL, 3LL, 2496LL);
    caps({20000, 30000, 12345}, 7, 10000, 500, 8908LL, 6LL, 130LL, 65536LL, 10LL, 17818LL);
    caps({1000000000, 1000000000, 1000000000}, 50, 10000, 10000, 60000000LL, 298507LL, 300006LL, 937500LL, 58595LL, 120000002LL);
    caps({2147483647, 2147483647, 2147483647, 1}, 50, 10000, 10000, 128849020LL, 641039LL, 644253LL, 2013265LL, 125831LL, 257698042LL);
    caps({2147483647, 2147483647}, 1, 10000, 10000, 4294967294LL, 429453LL, 429500LL, 67108863LL, 4194305LL, 8589934590LL);
    // record estimate
    est(0LL, "a.gz", 0LL);
    est(0LL, ".gz", 0LL);
    est(0LL, "x.paf.gz", 0LL);
    est(0LL, "x.paf", 0LL);
    est(0LL, "gz", 0LL);
    est(59LL, "a.gz", 3LL);
    est(59LL, ".gz", 0LL);
    est(59LL, "x.paf.gz", 3LL);
    est(59LL, "x.paf", 0LL);
    est(59LL, "gz", 0LL);
    est(60LL, "a.gz", 4LL);
    est(60LL, ".gz", 1LL);
    est(60LL, "x.paf.gz", 4LL);
    est(60LL, "x.paf", 1LL);
    est(60LL, "gz", 1LL);
    est(2800000000LL, "a.gz", 186666666LL);
    est(2800000000LL, ".gz", 46666666LL);
    est(2800000000LL, "x.paf.gz", 186666666LL);
    est(2800000000LL, "x.paf", 46666666LL);
    est(2800000000LL, "gz", 46666666LL);
    // few_sorted_runs
    few("ascending", 1LL, 0, true);
    few("descending", 1LL, 0, true);
    few("sampled3", 1LL, 0, true);
    few("sampled4", 1LL, 0, true);
    few("between3", 1LL, 0, true);
    few("between4", 1LL, 0, true);
    few("between40", 1LL, 0, true);
    few("ascending", 2LL, 0, true);
    few("descending", 2LL, 1, true);
    few("sampled3", 2LL, 1, true);
    few("sampled4", 2LL, 1, true);
    few("between3", 2LL, 0, true);
    few("between4", 2LL, 0, true);
    few("between40", 2LL, 0, true);
    few("ascending", 8192LL, 0, true);
    few("descending", 8192LL, 8191, false);
    few("sampled3", 8192LL, 3, true);
    few("sampled4", 8192LL, 4, false);
    few("between3", 8192LL, 3, true);
    few("between4", 8192LL, 4, false);
    few("between40", 8192LL, 40, false);
    few("ascending", 8193LL, 0, true);
    few("descending", 8193LL, 8192, false);
    few("sampled3", 8193LL, 3, true);
    few("sampled4", 8193LL, 4, false);
    few("between3", 8193LL, 3, true);
    few("between4", 8193LL, 4, false);
    few("between40", 8193LL, 40, false);
    few("ascending", 100000LL, 0, true);
    few("descending", 100000LL, 99999, false);
    few("sampled3", 100000LL, 3, true);
    few("sampled4", 100000LL, 4, false);
    few("between3", 100000LL, 3, true);
    few("between4", 100000LL, 4, true);
    few("between40", 100000LL, 40, true);
    // widths
    CHECK(byte_width(false, 0) == 1, "byte_width");
    CHECK(reserve_cov_width(false, false, 0) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, false, 0) == 1, "reserve_cov_width");
    CHECK(byte_width(false, 1) == 1, "byte_width");
    CHECK(reserve_cov_width(false, false, 1) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, false, 1) == 1, "reserve_cov_width");
    CHECK(byte_width(false, 39) == 1, "byte_width");
    CHECK(reserve_cov_width(false, false, 39) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, false, 39) == 1, "reserve_cov_width");
    CHECK(byte_width(false, 40) == 2, "byte_width");
    CHECK(reserve_cov_width(false, false, 40) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, false, 40) == 2, "reserve_cov_width");
    CHECK(byte_width(false, 41) == 2, "byte_width");
    CHECK(reserve_cov_width(false, false, 41) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, false, 41) == 2, "reserve_cov_width");
    CHECK(byte_width(true, 0) == 2, "byte_width");
    CHECK(reserve_cov_width(false, true, 0) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, true, 0) == 2, "reserve_cov_width");
    CHECK(byte_width(true, 1) == 2, "byte_width");
    CHECK(reserve_cov_width(false, true, 1) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, true, 1) == 2, "reserve_cov_width");
    CHECK(byte_width(true, 39) == 2, "byte_width");
    CHECK(reserve_cov_width(false, true, 39) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, true, 39) == 2, "reserve_cov_width");
    CHECK(byte_width(true, 40) == 2, "byte_width");
    CHECK(reserve_cov_width(false, true, 40) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, true, 40) == 2, "reserve_cov_width");
    CHECK(byte_width(true, 41) == 2, "byte_width");
    CHECK(reserve_cov_width(false, true, 41) == 8, "reserve_cov_width");
    CHECK(reserve_cov_width(true, true, 41) == 2, "reserve_cov_width");
    CHECK(first_cov_width(0, false, false, 0, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(0, false, false, 0, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(0, false, false, 2, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(0, false, false, 2, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(0, false, true, 0, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(0, false, true, 0, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(0, false, true, 2, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(0, false, true, 2, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(0, true, false, 0, 39) == 8, "first_cov_width");
    CHECK(first_cov_width(0, true, false, 0, 40) == 8, "first_cov_width");
    CHECK(first_cov_width(0, true, false, 2, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(0, true, false, 2, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(0, true, true, 0, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(0, true, true, 0, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(0, true, true, 2, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(0, true, true, 2, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(1, false, false, 0, 39) == 8, "first_cov_width");
    CHECK(first_cov_width(1, false, false, 0, 40) == 8, "first_cov_width");
    CHECK(first_cov_width(1, false, false, 2, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(1, false, false, 2, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(1, false, true, 0, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(1, false, true, 0, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(1, false, true, 2, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(1, false, true, 2, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(1, true, false, 0, 39) == 8, "first_cov_width");
    CHECK(first_cov_width(1, true, false, 0, 40) == 8, "first_cov_width");
    CHECK(first_cov_width(1, true, false, 2, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(1, true, false, 2, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(1, true, true, 0, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(1, true, true, 0, 40) == 2, "first_cov_width");
    CHECK(first_cov_width(1, true, true, 2, 39) == 1, "first_cov_width");
    CHECK(first_cov_width(1, true, true, 2, 40) == 2, "first_cov_width");
    // ladder
    step(8, 65536LL, 125000LL, 1000000LL, 8, 125000LL);
    step(8, 65536LL, 125001LL, 1000000LL, 2, 65536LL);
    step(1, 65536LL, 62500LL, 1000000LL, 1, 62500LL);
    step(1, 65536LL, 62501LL, 1000000LL, 2, 65536LL);
    step(1, 65536LL, 125001LL, 1000000LL, 2, 65536LL);
    step(2, 65536LL, 62501LL, 1000000LL, 2, 62501LL);
    step(2, 65536LL, 999999LL, 1000000LL, 2, 999999LL);
    step(8, 65536LL, 70000LL, 7LL, 2, 65536LL);
    step(1, 65536LL, 70000LL, 15LL, 2, 65536LL);
    step(1, 65536LL, 70000LL, 0LL, 2, 65536LL);
    CHECK(ladder_stops(0, 0, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(0, 0, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(0, 0, 65537LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(0, 1, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(0, 1, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(0, 1, 65537LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(0, 2, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(0, 2, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(0, 2, 65537LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(8, 0, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(8, 0, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(8, 0, 65537LL, 65536LL) == false, "ladder_stops");
    CHECK(ladder_stops(8, 1, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(8, 1, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(8, 1, 65537LL, 65536LL) == false, "ladder_stops");
    CHECK(ladder_stops(8, 2, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(8, 2, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(8, 2, 65537LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 0, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 0, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 0, 65537LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 1, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 1, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 1, 65537LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 2, 65535LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 2, 65536LL, 65536LL) == true, "ladder_stops");
    CHECK(ladder_stops(3, 2, 65537LL, 65536LL) == true, "ladder_stops");
    // the bytes of the coverage array an attempt writes, and whether the page-locked range holds them: -e below 40 locks
    // (n_win + 1) bytes beside the tokenising, which holds a first attempt in bytes or four-bit steps and no attempt in two bytes
    CHECK(cov_bytes_needed(1, 132300LL) == 132301LL, "cov_bytes_needed");
    CHECK(cov_bytes_needed(2, 132300LL) == 264602LL, "cov_bytes_needed");
    CHECK(cov_bytes_needed(8, 132300LL) == 66150LL, "cov_bytes_needed");
    CHECK(cov_bytes_needed(8, 132301LL) == 66151LL, "cov_bytes_needed");
    CHECK(cov_bytes_needed(1, 0LL) == 1LL && cov_bytes_needed(2, 0LL) == 2LL && cov_bytes_needed(8, 0LL) == 0LL, "cov_bytes_needed");
    CHECK(cov_bytes_needed(2, 3000000000LL) == 6000000002LL, "cov_bytes_needed beyond 32 bits");
    for (long long n_win : {0LL, 1LL, 132300LL, 3000000000LL}) {
        const Capacities c0 = output_capacities(0, nullptr, 50, 2000, 1000);
        CHECK(c0.cov8_bytes == 2, "an empty job's coverage array");
        for (int w : {1, 2, 8}) CHECK(cov_bytes_needed(w, n_win) <= (n_win + 1) * 2, "the array as allocated holds width %d of %lld windows", w, n_win);
        const long long one = cov_bytes_needed(byte_width(false, 39), n_win), two = cov_bytes_needed(byte_width(false, 40), n_win);
        CHECK(cov_range_too_short(1, n_win, one) == false, "a byte per window in the range locked for it");
        CHECK(cov_range_too_short(8, n_win, one) == false, "four-bit steps in the range locked for a byte");
        CHECK(cov_range_too_short(2, n_win, one) == true, "two bytes per window leave the range locked for one");
        CHECK(cov_range_too_short(2, n_win, two) == false && cov_range_too_short(1, n_win, two) == false && cov_range_too_short(8, n_win, two) == false,
              "nothing leaves the range locked for two");
        CHECK(cov_range_too_short(2, n_win, two - 1) == true && cov_range_too_short(1, n_win, one - 1) == true, "one byte short");
        CHECK(cov_range_too_short(1, n_win, 0) == true && cov_range_too_short(2, n_win, 0) == true, "nothing locked yet");
    }
    // start time
    CHECK(stat_start_time("4242 (raft) S 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21 2200 23 24 25") == 2200ULL, "stat_start_time");
    CHECK(stat_start_time("4242 (a b) S 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21 2200 23 24 25") == 2200ULL, "stat_start_time");
    CHECK(stat_start_time("4242 (x) y (z) S 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21 2200 23 24 25") == 2200ULL, "stat_start_time");
    CHECK(stat_start_time("4242 (raft) S 3 4 5") == 0ULL, "stat_start_time");
    CHECK(stat_start_time("no parenthesis at all 1 2 3") == 0ULL, "stat_start_time");
    CHECK(stat_start_time("") == 0ULL, "stat_start_time");
    // labels
    CHECK(strcmp(input_label(0, false, 0, false), "columns") == 0, "input_label");
    CHECK(strcmp(input_label(0, false, 0, true), "columns (offsets and window records derived by the engine)") == 0, "input_label");
    CHECK(strcmp(input_label(0, false, 2, false), "grouped") == 0, "input_label");
    CHECK(strcmp(input_label(0, false, 2, true), "grouped") == 0, "input_label");
    CHECK(strcmp(input_label(0, true, 0, false), "windows") == 0, "input_label");
    CHECK(strcmp(input_label(0, true, 0, true), "windows") == 0, "input_label");
    CHECK(strcmp(input_label(0, true, 2, false), "windows") == 0, "input_label");
    CHECK(strcmp(input_label(0, true, 2, true), "windows") == 0, "input_label");
    CHECK(strcmp(input_label(2, false, 0, false), "pre-split slices (one exchange step)") == 0, "input_label");
    CHECK(strcmp(input_label(2, false, 0, true), "pre-split slices (one exchange step)") == 0, "input_label");
    CHECK(strcmp(input_label(2, false, 2, false), "pre-split slices (one exchange step)") == 0, "input_label");
    CHECK(strcmp(input_label(2, false, 2, true), "pre-split slices (one exchange step)") == 0, "input_label");
    CHECK(strcmp(input_label(2, true, 0, false), "pre-split slices (one exchange step)") == 0, "input_label");
    CHECK(strcmp(input_label(2, true, 0, true), "pre-split slices (one exchange step)") == 0, "input_label");
    CHECK(strcmp(input_label(2, true, 2, false), "pre-split slices (one exchange step)") == 0, "input_label");
    CHECK(strcmp(input_label(2, true, 2, true), "pre-split slices (one exchange step)") == 0, "input_label");
    CHECK(strcmp(encoding_label(8), "delta4") == 0, "encoding_label");
    CHECK(strcmp(encoding_label(2), "uint16") == 0, "encoding_label");
    CHECK(strcmp(encoding_label(1), "uint8") == 0, "encoding_label");
    return cli_check::finish("cli_plan_check");
}
