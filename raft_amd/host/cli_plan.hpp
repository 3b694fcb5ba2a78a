// cli_plan.hpp -- what the `raft` command line (raft_main.cpp) decides, as plain functions over plain values: which devices a job
// runs on, how large the arrays are that its results come back in, which coverage encoding it asks for first and what it asks for
// after an overflow of the exception list, and the two descriptions on the stage clock.  No getenv, no file, no thread, nothing
// of raft_hip.h but its constants: a host compiler alone builds it (tests/cli_plan_check.cpp does, under the sanitizers).
#pragma once
#include "../../include/raft_hip.h"
#include "../../include/raft_hip_low.h"
#include "../../include/raft_host_end.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace raft_cli {

// RAFT_DEVICES=0,1,...: the GPUs of the node that share the job (reads shard across them, host-routed, no collective;
// SURVEY.md §8e); RAFT_DEVICE=n: a single one; default: device 0.  A device may be named twice.  The list ends at the first
// thing that is not a number, a trailing comma included.
// RAFT_RANKS=N: the PRE-SPLIT job (BASELINE configs[3]): the record stream is cut into N contiguous slices, rank r
// -- a context on device r modulo the devices named -- holds slice r, and ONE exchange step routes every interval to the rank
// that owns its read (raft_hip_run_presplit_local).  Outputs are the single-rank run's, byte for byte.  ranks = 0: not such a job.
struct DeviceList {
    std::vector<int> devices;
    int ranks = 0;
};

inline DeviceList device_list(const char *devices_text, const char *device_text, const char *ranks_text)
{
    DeviceList l;
    if (const char *e = devices_text) {
        for (const char *q = e; *q;) {
            char *end = nullptr;
            const long v = strtol(q, &end, 10);
            if (end == q) break;
            l.devices.push_back((int)v);
            q = (*end == ',') ? end + 1 : end;
            if (*end != ',' && *end != '\0') break;
        }
    }
    if (l.devices.empty()) l.devices.push_back(device_text ? atoi(device_text) : 0);
    l.ranks = ranks_text ? std::max(1, std::min(64, atoi(ranks_text))) : 0;
    if (l.ranks > 0) {
        const std::vector<int> named = l.devices;
        l.devices.clear();
        for (int r = 0; r < l.ranks; ++r) l.devices.push_back(named[(size_t)r % named.size()]);
    }
    return l;
}

// Host arrays for everything that comes back, sized by the bounds of raft_hip.h (from the read lengths alone): windows, repeats,
// fragments, the first size of the exception list, the block anchors of the four-bit step encoding, and the bytes of the coverage
// array (two per window: room for either byte encoding).
struct Capacities {
    int64_t n_win = 0, rep_cap = 0, frag_cap = 0, exc_cap0 = 0, n_anchor = 0, cov8_bytes = 0;
};

inline Capacities output_capacities(int32_t n_reads, const int32_t *read_len, int reso, int repeat_length, int interval_length)
{
    Capacities c;
    const int64_t minw = std::max<int64_t>(((int64_t)repeat_length + reso - 1) / reso, 1);
    int64_t sum_len = 0;
    for (int32_t i = 0; i < n_reads; ++i) { c.n_win += ((int64_t)read_len[i] + reso - 1) / reso; sum_len += read_len[i]; }
    c.rep_cap = (c.n_win + n_reads) / (minw + 1);
    c.frag_cap = sum_len / interval_length + 2 * (int64_t)n_reads;
    c.exc_cap0 = std::max<int64_t>(1 << 16, c.n_win / 64);
    c.n_anchor = c.n_win / 1024 + 2;
    c.cov8_bytes = (c.n_win + 1) * 2;
    return c;
}

// The record count to within a few per cent from the size of the overlaps file: a PAF line of hifiasm's has ~63 bytes; .gz: ~4x
// that when inflated.
inline int64_t record_estimate(int64_t file_size, const std::string &name)
{
    const bool gz = name.size() > 3 && name.compare(name.size() - 3, 3, ".gz") == 0;
    return file_size * (gz ? 4 : 1) / 60;
}

// Handing over the plain columns, the CLI does not know the stream's shape exactly; 8 k samples tell a handful of sorted runs --
// which the engine cuts into chunks wherever it likes -- from a shuffled stream, whose routed chunks end where the host's buckets
// do and keep the byte encodings.  A sample is compared with the sample before it; few: fewer than four descents.
inline bool few_sorted_runs(const int32_t *qid, int64_t n_rec)
{
    const int64_t S = std::min<int64_t>(n_rec, 8192);
    int descents = 0;
    int64_t prev = 0;
    for (int64_t i = 1; i < S; ++i) {
        const int64_t pos = i * (n_rec - 1) / (S - 1);
        if (qid[pos] < qid[prev]) ++descents;
        prev = pos;
    }
    return descents < 4;
}

// One byte per window unless the expected coverage lets repeats pile up beyond it (from 40x on: two); -e auto, while the depth
// is not known yet: two.
inline int byte_width(bool auto_cov, int est_cov) { return auto_cov || est_cov >= 40 ? 2 : 1; }

// The bytes of the coverage array an attempt in `cov_width` writes: one or two per window, or a four-bit step per window.  The
// array is allocated for the widest of them (Capacities::cov8_bytes); it is page-locked for the first attempt's byte encoding
// beside the tokenising, and an attempt that needs more than is page-locked registers the array anew (a copy that leaves a
// registered range is an invalid argument to the runtime; the same copy into memory that is not registered at all is not).
inline int64_t cov_bytes_needed(int cov_width, int64_t n_win)
{
    return cov_width == RAFT_HIP_COV_DELTA4 ? (n_win + 1) / 2 : (n_win + 1) * (int64_t)cov_width;
}

inline bool cov_range_too_short(int cov_width, int64_t n_win, int64_t bytes_locked) { return cov_bytes_needed(cov_width, n_win) > bytes_locked; }

// What the device buffers are reserved for before the overlaps are tokenised: what a hifiasm-shaped PAF will use.
inline int reserve_cov_width(bool no_delta4, bool auto_cov, int est_cov) { return no_delta4 ? byte_width(auto_cov, est_cov) : RAFT_HIP_COV_DELTA4; }

// The job's first encoding.  Grouped input (whose chunks the pipelines can cut where they like) brings the coverage back as
// four-bit steps: the step from one window to the next is the pileup's own difference array, within +-7 for all but a few windows
// in a thousand whatever the depth -- half of a byte per window, a quarter of two.  Any other stream: the byte encodings.
inline int first_cov_width(int n_runs, bool few_runs, bool no_delta4, int ranks, int est_cov)
{
    return ((n_runs > 0 || few_runs) && !no_delta4 && ranks == 0) ? RAFT_HIP_COV_DELTA4 : byte_width(false, est_cov);
}

// The width a context has outside the survey: 4 unless RAFT_COV_WIDTH (the test sweeps' variable, read by the engine) chose.
inline int context_cov_width(const char *cov_width_text)
{
    const int was = cov_width_text ? atoi(cov_width_text) : 4;
    return (was == 1 || was == 2 || was == RAFT_HIP_COV_DELTA4) ? was : 4;
}

// The ladder: an attempt that met more windows at or above the limit than the list holds (n_exc says how many) is followed by
// one with two bytes per window when a byte leaves more than one window in 16 on the list (four-bit steps: one in 8 -- steps that
// mostly do not fit are not a coverage profile), else by one with room for exactly those.  Three attempts at the most.
struct Attempt {
    int cov_width;
    int64_t exc_cap;
};

inline bool ladder_stops(int rc, int attempt, int64_t n_exc, int64_t exc_cap)
{
    return rc != RAFT_HIP_ERR_TOO_LARGE || attempt == 2 || n_exc <= exc_cap;
}

inline Attempt next_attempt(int cov_width, int64_t exc_cap, int64_t n_exc, int64_t n_win)
{
    if (cov_width == RAFT_HIP_COV_DELTA4 && n_exc > n_win / 8) return {2, exc_cap};
    if (cov_width == 1 && n_exc > n_win / 16) return {2, exc_cap};
    return {cov_width, n_exc};
}

// --low-cov C: C is a whole number >= 0 written in digits alone (no sign, no blank, nothing behind it), at most INT32_MAX.
inline bool parse_low_cov(const char *text, int32_t *low_cov)
{
    if (!text || !*text) return false;
    int64_t v = 0;
    for (const char *q = text; *q; ++q) {
        if (*q < '0' || *q > '9') return false;
        v = v * 10 + (*q - '0');
        if (v > INT32_MAX) return false;
    }
    *low_cov = (int32_t)v;
    return true;
}

// --repeat-overlaps A: A (min_anchor of raft_hip_repeat_overlaps_*) is a whole number >= 1 written in digits alone, at most INT32_MAX.
inline bool parse_min_anchor(const char *text, int32_t *min_anchor)
{
    int32_t v = 0;
    if (!parse_low_cov(text, &v) || v < 1) return false;
    *min_anchor = v;
    return true;
}

// --fragment-overlaps: the option's stdout line, the last one, from raft_hip_frag_summary's counts
inline std::string fragment_overlaps_line(int64_t fragments, int64_t spanned, int64_t contained, int64_t contained_repeat, int64_t reads_whole,
                                          int64_t reads_all, int32_t n_reads)
{
    return "INFO, fragment_overlaps(), fragments = " + std::to_string(fragments) + ", spanned = " + std::to_string(spanned) + ", contained = " +
           std::to_string(contained) + ", contained with repeat = " + std::to_string(contained_repeat) + ", reads spanned whole = " +
           std::to_string(reads_whole) + ", reads with every fragment contained = " + std::to_string(reads_all) + " of " + std::to_string(n_reads);
}

// --repeat-stats: the threshold of the table's high windows is the job's high_cov (repeat.hpp:89-90), at least 1
inline int32_t repeat_stats_threshold(int est_cov, double cov_mul)
{
    const int32_t high_cov = (int32_t)(est_cov * cov_mul);
    return high_cov > 1 ? high_cov : 1;
}

// ... its stdout line, behind the line of --fragment-overlaps, from raft_hip_rst_summary's counts
inline std::string repeat_stats_line(int64_t runs, int64_t interior, int64_t spanned, int64_t interior_spanned, int64_t touched, int64_t sides_inside)
{
    return "INFO, repeat_stats(), repeats = " + std::to_string(runs) + ", interior = " + std::to_string(interior) + ", spanned = " +
           std::to_string(spanned) + ", interior spanned = " + std::to_string(interior_spanned) + ", untouched = " + std::to_string(runs - touched) +
           ", sides inside a repeat = " + std::to_string(sides_inside);
}

// --min-identity PCT: digits with at most one decimal digit ("99", "99.5", "100", "0.1"), 0 < PCT <= 100, into per mille (the
// min_identity_permille of raft_hip_filter_overlaps_*).  No sign, no blank, no exponent, nothing behind a point but one digit, and no
// strtod: the text is the number.
inline bool parse_min_identity(const char *text, int32_t *permille)
{
    if (!text || *text < '0' || *text > '9') return false;
    int64_t v = 0;
    const char *q = text;
    for (; *q >= '0' && *q <= '9'; ++q) {
        v = v * 10 + (*q - '0');
        if (v > 100) return false;
    }
    v *= 10;
    if (*q == '.') {
        if (q[1] < '0' || q[1] > '9') return false;
        v += q[1] - '0';
        q += 2;
    }
    if (*q || v < 1 || v > 1000) return false;
    *permille = (int32_t)v;
    return true;
}

// --min-overlap BASES: BASES (min_span of raft_hip_filter_overlaps_*) is a whole number >= 1 written in digits alone, at most INT32_MAX.
inline bool parse_min_overlap(const char *text, int32_t *min_span) { return parse_min_anchor(text, min_span); }

// ... the options' stdout line, directly behind the reference's own last line and before the lines of the other options, from
// raft_hip_flt_summary's counts
inline std::string filter_overlaps_line(int32_t permille, int32_t min_span, int64_t records, int64_t kept, int64_t below_identity, int64_t below_span)
{
    return "INFO, filter_overlaps(), min_identity = " + std::to_string(permille) + " per mille, min_overlap = " + std::to_string(min_span) +
           ", records = " + std::to_string(records) + ", kept = " + std::to_string(kept) + ", below identity = " + std::to_string(below_identity) +
           ", below overlap = " + std::to_string(below_span);
}

// --overlap-ends H: H (max_overhang of raft_hip_overlap_ends_*) is a whole number >= 0 written in digits alone, at most INT32_MAX.
inline bool parse_overlap_ends(const char *text, int32_t *max_overhang) { return parse_low_cov(text, max_overhang); }

// --ends-min-ratio F: F (min_ratio_permille) is a whole number written in digits alone, 0 .. 1000; without the option it is
constexpr int32_t kEndsMinRatioDefault = 800;
inline bool parse_ends_min_ratio(const char *text, int32_t *permille)
{
    int32_t v = 0;
    if (!parse_low_cov(text, &v) || v > 1000) return false;
    *permille = v;
    return true;
}

// ... the option's stdout line, the last one, from raft_hip_end_summary's counts (dead ends: the reads with status dead5 or dead3)
inline std::string overlap_ends_line(int32_t max_overhang, int32_t min_ratio, int64_t records, int64_t internal, int64_t query_contained,
                                     int64_t target_contained, int64_t dovetail, int64_t self, int64_t invalid, int64_t reads_contained,
                                     int64_t dead_ends, int64_t reads_isolated, int32_t n_reads)
{
    return "INFO, overlap_ends(), max_overhang = " + std::to_string(max_overhang) + ", min_ratio = " + std::to_string(min_ratio) +
           " per mille, records = " + std::to_string(records) + ", internal = " + std::to_string(internal) + ", query contained = " +
           std::to_string(query_contained) + ", target contained = " + std::to_string(target_contained) + ", dovetail = " + std::to_string(dovetail) +
           ", self = " + std::to_string(self) + ", invalid = " + std::to_string(invalid) + ", contained reads = " + std::to_string(reads_contained) +
           ", dead ends = " + std::to_string(dead_ends) + ", isolated reads = " + std::to_string(reads_isolated) + " of " + std::to_string(n_reads);
}

// --best-overlaps: the option's stdout line, the last one (behind overlap_ends'), from raft_hip_best_summary's counts
inline std::string best_overlaps_line(int64_t records, int64_t candidates, int64_t left_out, int64_t ends_best, int64_t ends_mutual,
                                      int64_t reads_both_mutual, int64_t reads_no_best, int64_t reads_skipped, int32_t n_reads)
{
    return "INFO, best_overlaps(), records = " + std::to_string(records) + ", candidates = " + std::to_string(candidates) + ", left out = " +
           std::to_string(left_out) + ", ends with a best overlap = " + std::to_string(ends_best) + ", mutual = " + std::to_string(ends_mutual) +
           ", reads with both ends mutual = " + std::to_string(reads_both_mutual) + ", reads without a best overlap = " + std::to_string(reads_no_best) +
           ", reads left out = " + std::to_string(reads_skipped) + " of " + std::to_string(n_reads);
}

// --unitigs: N50 of the unitigs, singletons included: the smallest length L such that the unitigs of length >= L hold at least half of the
// total -- sorted descending, the length at the first prefix with 2 * cum >= total; 0 for no unitigs.
inline int64_t unitig_n50(const int64_t *lengths, int64_t n)
{
    if (n <= 0 || !lengths) return 0;
    std::vector<int64_t> v(lengths, lengths + n);
    std::sort(v.begin(), v.end(), [](int64_t a, int64_t b) { return a > b; });
    int64_t total = 0, cum = 0;
    for (int64_t x : v) total += x;
    for (int64_t x : v) {
        cum += x;
        if (cum >= total - cum) return x;
    }
    return v.back();
}

// ... the option's stdout line, the last one (behind best_overlaps'), from raft_hip_utg_summary's counts and the N50
inline std::string unitigs_line(int64_t reads, int64_t skipped, int64_t unitigs, int64_t singletons, int64_t circular, int64_t longest_reads,
                                int64_t longest_length, int64_t total_length, int64_t n50)
{
    return "INFO, unitigs(), reads = " + std::to_string(reads) + ", left out = " + std::to_string(skipped) + ", unitigs = " + std::to_string(unitigs) +
           ", singletons = " + std::to_string(singletons) + ", circular = " + std::to_string(circular) + ", longest = " + std::to_string(longest_reads) +
           " reads, longest length = " + std::to_string(longest_length) + ", total length = " + std::to_string(total_length) +
           ", N50 = " + std::to_string(n50);
}

// --components: the option's stdout line, behind unitigs' and before fragment_paf's, from raft_hip_cc_summary's counts (kinds: the mask)
inline std::string components_line(int32_t kind_mask, int64_t records, int64_t edges, int64_t components, int64_t singletons, int64_t largest_reads,
                                   int64_t largest_bases, int64_t total_bases, int64_t permille, int64_t n_reads)
{
    return "INFO, components(), kinds = " + std::to_string(kind_mask) + ", records = " + std::to_string(records) + ", edges = " + std::to_string(edges) +
           ", components = " + std::to_string(components) + ", singletons = " + std::to_string(singletons) + ", largest = " + std::to_string(largest_reads) +
           " reads, largest bases = " + std::to_string(largest_bases) + " of " + std::to_string(total_bases) + ", reads in the largest = " +
           std::to_string(permille) + " per mille of " + std::to_string(n_reads);
}

// --string-graph-fuzz Z: Z (fuzz of raft_hip_string_graph_*) is a whole number >= 0 written in digits alone, at most INT32_MAX; without the
// option it is miniasm's gap fuzz
constexpr int32_t kStringGraphFuzzDefault = 1000;
inline bool parse_string_graph_fuzz(const char *text, int32_t *fuzz) { return parse_low_cov(text, fuzz); }

// The edge list's first size: a string graph keeps about an edge per read -- two per read where most ends branch --, and never more
// than two per record; at least 1, so that the arrays are there.  The call says what it needs when that is not enough.
inline int64_t string_graph_capacity0(int64_t n_rec, int32_t n_reads)
{
    return std::max<int64_t>(1, std::min<int64_t>(2 * n_rec, 2 * (int64_t)n_reads + 1024));
}

// --string-graph: the option's stdout line, behind components' and before fragment_paf's, from raft_hip_sg_summary's counts
inline std::string string_graph_line(int32_t fuzz, int64_t records, int64_t views, int64_t left_out, int64_t arcs, int64_t duplicates, int64_t unpaired,
                                     int64_t reducible, int64_t edges, int64_t kept_edges, int64_t ends_one, int64_t ends_more, int64_t ends_dead,
                                     int64_t ends_mutual, int64_t reads_flagged, int64_t longest_row, int64_t n_reads)
{
    return "INFO, string_graph(), fuzz = " + std::to_string(fuzz) + ", records = " + std::to_string(records) + ", dovetail views = " + std::to_string(views) +
           ", left out = " + std::to_string(left_out) + ", arcs = " + std::to_string(arcs) + ", duplicates = " + std::to_string(duplicates) +
           ", unpaired = " + std::to_string(unpaired) + ", reducible = " + std::to_string(reducible) + ", edges = " + std::to_string(edges) +
           ", kept = " + std::to_string(kept_edges) + ", ends with one = " + std::to_string(ends_one) + ", ends that branch = " + std::to_string(ends_more) +
           ", dead ends = " + std::to_string(ends_dead) + ", mutual ends = " + std::to_string(ends_mutual) + ", reads left out = " +
           std::to_string(reads_flagged) + " of " + std::to_string(n_reads) + ", longest row = " + std::to_string(longest_row);
}

// --containment: the option's stdout line, behind string_graph's and before fragment_paf's, from raft_hip_ctn_summary's counts
inline std::string containment_line(int64_t records, int64_t views, int64_t not_longer, int64_t with_parent, int64_t orphans, int64_t roots,
                                    int64_t roots_with_tree, int64_t deepest, int64_t largest_reads, int64_t largest_bases)
{
    return "INFO, containment(), records = " + std::to_string(records) + ", containment views = " + std::to_string(views) + ", not longer = " +
           std::to_string(not_longer) + ", reads with a parent = " + std::to_string(with_parent) + ", contained without a parent = " +
           std::to_string(orphans) + ", roots = " + std::to_string(roots) + ", roots with a tree = " + std::to_string(roots_with_tree) +
           ", deepest = " + std::to_string(deepest) + ", largest tree = " + std::to_string(largest_reads) + " reads, largest tree bases = " +
           std::to_string(largest_bases);
}

// ... and, with --unitigs, the line behind it, from raft_hip_place_summary's counts
inline std::string place_contained_line(int64_t unitigs, int64_t placed, int64_t unplaced, int64_t n_reads, int64_t gained, int64_t greatest_permille)
{
    return "INFO, place_contained(), unitigs = " + std::to_string(unitigs) + ", placed = " + std::to_string(placed) + ", unplaced = " +
           std::to_string(unplaced) + " of " + std::to_string(n_reads) + ", unitigs that gained reads = " + std::to_string(gained) +
           ", greatest depth = " + std::to_string(greatest_permille) + " per mille";
}

// --graph-clean: the string graph of --string-graph without its weak edges and its tips (raft_hip_graph_clean_host), and the unitigs of
// what is left.  --clean-min-ratio W: W (min_ratio_permille) is a whole number written in digits alone, 0 .. 1000; without the option it
// is miniasm's lower overlap drop ratio.  --clean-tip-reads T: T (max_tip_reads) is a whole number >= 0 in digits alone, at most
// INT32_MAX; without the option it is miniasm's max_ext.  --clean-rounds R: R (rounds) is a whole number in digits alone, 1 .. 64.
constexpr int32_t kCleanMinRatioDefault = 500, kCleanTipReadsDefault = 4, kCleanRoundsDefault = 3, kCleanRoundsMax = 64;
inline bool parse_clean_min_ratio(const char *text, int32_t *permille) { return parse_ends_min_ratio(text, permille); }
inline bool parse_clean_tip_reads(const char *text, int32_t *reads) { return parse_low_cov(text, reads); }
inline bool parse_clean_rounds(const char *text, int32_t *rounds)
{
    int32_t v = 0;
    if (!parse_low_cov(text, &v) || v < 1 || v > kCleanRoundsMax) return false;
    *rounds = v;
    return true;
}

// ... the option's two stdout lines, behind every other option's, from raft_hip_cln_summary's counts and from raft_hip_utg_summary's
inline std::string graph_clean_line(int32_t min_ratio, int32_t tip_reads, int64_t rounds_run, int32_t rounds, int64_t converged, int64_t edges,
                                    int64_t weak_edges, int64_t tips, int64_t tip_reads_fallen, int64_t tip_bases, int64_t tip_edges, int64_t kept_edges,
                                    int64_t ends_more, int64_t ends_dead, int64_t isolated_short)
{
    return "INFO, graph_clean(), min_ratio = " + std::to_string(min_ratio) + " per mille, tip_reads = " + std::to_string(tip_reads) + ", rounds = " +
           std::to_string(rounds_run) + " of " + std::to_string(rounds) + ", converged = " + std::to_string(converged) + ", edges = " + std::to_string(edges) +
           ", weak edges = " + std::to_string(weak_edges) + ", tips = " + std::to_string(tips) + ", tip reads = " + std::to_string(tip_reads_fallen) +
           ", tip bases = " + std::to_string(tip_bases) + ", tip edges = " + std::to_string(tip_edges) + ", kept edges = " + std::to_string(kept_edges) +
           ", ends that branch = " + std::to_string(ends_more) + ", dead ends = " + std::to_string(ends_dead) + ", short isolated chains = " +
           std::to_string(isolated_short);
}
inline std::string graph_clean_unitigs_line(int64_t reads, int64_t skipped, int64_t unitigs, int64_t singletons, int64_t circular, int64_t longest_reads,
                                            int64_t longest_length, int64_t total_length, int64_t n50)
{
    const std::string fields = unitigs_line(reads, skipped, unitigs, singletons, circular, longest_reads, longest_length, total_length, n50);
    return "INFO, graph_clean_unitigs()" + fields.substr(std::string("INFO, unitigs()").size());
}

// --fragment-paf: PREFIX.fragments.paf, the job's overlaps lifted onto its fragments (raft_hip_lift_overlaps_host).
// --fragment-paf-min L: L (min_len of that call) is a whole number >= 1 written in digits alone, at most INT32_MAX; without the option it is
constexpr int32_t kFragmentPafMinDefault = 1;
inline bool parse_fragment_paf_min(const char *text, int32_t *min_len) { return parse_min_anchor(text, min_len); }

// ... the option's stdout line, the last one of all, from raft_hip_lift_summary's counts
inline std::string fragment_paf_line(int32_t min_len, int64_t records, int64_t lifted, int64_t cut, int64_t none, int64_t dropped, int64_t most)
{
    return "INFO, fragment_paf(), min_len = " + std::to_string(min_len) + ", records = " + std::to_string(records) + ", lifted = " + std::to_string(lifted) +
           ", cut = " + std::to_string(cut) + ", without a fragment pair = " + std::to_string(none) + ", dropped pairs = " + std::to_string(dropped) +
           ", most from one record = " + std::to_string(most);
}

// What the command line says, as parse_options (raft_main.cpp) leaves it: the reference's parameters (param.hpp:18-31; -e auto: est_cov
// is read from the data before the job), and one value per long option of this program's own -- kLongOptions says what each asks for.
struct Options {
    int reso = 50, est_cov = 0;
    double cov_mul = 1.5;
    int repeat_length = 10000, interval_length = 10000, read_length = 20000, overlap_length = 500, flanking_length = 1000;
    std::string prefix = "raft";
    bool auto_cov = false;
    bool read_stats = false, fragment_overlaps = false, repeat_stats = false, best_overlaps = false, unitigs = false, fragment_paf = false;
    bool components = false, string_graph = false;
    int32_t low_cov = -1, overlap_ends = -1;                            // -1: not asked for
    int32_t min_anchor = 0, min_identity = 0, min_overlap = 0;          // 0: not asked for; the identity in per mille
    int32_t ends_min_ratio = kEndsMinRatioDefault, fragment_paf_min = kFragmentPafMinDefault;
    bool ends_ratio_given = false, fragment_paf_min_given = false;
    int32_t string_graph_fuzz = kStringGraphFuzzDefault;
    bool string_graph_fuzz_given = false;
    bool containment = false;
    bool graph_clean = false;
    int32_t clean_min_ratio = kCleanMinRatioDefault, clean_tip_reads = kCleanTipReadsDefault, clean_rounds = kCleanRoundsDefault;
    bool clean_min_ratio_given = false, clean_tip_reads_given = false, clean_rounds_given = false;
};

// The long options, one row each: the text's parser (none: a flag, which takes no argument), the value it writes, and the flag
// that is set -- the option itself for a flag, the "given" mark of a value that has one.  The short options are the reference's and
// stay a switch in parse_options, quirks and all.
struct LongOption { const char *name; bool (*parse)(const char *, int32_t *); int32_t Options::*value; bool Options::*flag; };

inline constexpr LongOption kLongOptions[] = {
    {"read-stats", nullptr, nullptr, &Options::read_stats},                 // PREFIX.read_stats.tsv, the per-read table (raft_hip_read_stats, raft_hip_census_host)
    {"low-cov", parse_low_cov, &Options::low_cov, nullptr},                 // C: PREFIX.low_coverage.bed, the runs of windows with coverage <= C (raft_hip_low_coverage)
    {"repeat-overlaps", parse_min_anchor, &Options::min_anchor, nullptr},   // A: PREFIX.repeat_overlaps.tsv and .records.tsv (raft_hip_repeat_overlaps_host)
    {"fragment-overlaps", nullptr, nullptr, &Options::fragment_overlaps},   // PREFIX.fragments.tsv, the fragments against the overlaps (raft_hip_frag_overlaps_host)
    {"repeat-stats", nullptr, nullptr, &Options::repeat_stats},             // PREFIX.long_repeats.stats.tsv, one line per repeat run (raft_hip_repeat_stats_host)
    {"min-identity", parse_min_identity, &Options::min_identity, nullptr},  // PCT, and --min-overlap BASES: only the records that pass go into the job
    {"min-overlap", parse_min_overlap, &Options::min_overlap, nullptr},     // (raft_hip_filter_overlaps_host, before anything else sees the stream)
    {"overlap-ends", parse_overlap_ends, &Options::overlap_ends, nullptr},  // H: PREFIX.overlap_ends.tsv, the kind of every record and the ends of every read
    {"ends-min-ratio", parse_ends_min_ratio, &Options::ends_min_ratio, &Options::ends_ratio_given},   // F, in per mille
    {"best-overlaps", nullptr, nullptr, &Options::best_overlaps},           // PREFIX.best_overlaps.tsv, the best overlap of every read end under --overlap-ends' H and F
    {"unitigs", nullptr, nullptr, &Options::unitigs},                       // PREFIX.unitigs.tsv and .unitigs.layout.tsv, the chains and cycles of --best-overlaps' mutual ends
    {"fragment-paf", nullptr, nullptr, &Options::fragment_paf},             // PREFIX.fragments.paf, the job's overlaps lifted onto its fragments (raft_hip_lift_overlaps_host)
    {"fragment-paf-min", parse_fragment_paf_min, &Options::fragment_paf_min, &Options::fragment_paf_min_given},   // L: pairs shorter than L on either side are dropped
};

// That table is closed at the thirteen; the options that came later stand here, rows of the same type, and the next one is a row here.
// long_option(k) counts through both: what getopt_long's array is built from and what a row it found is applied with.
inline constexpr LongOption kLaterLongOptions[] = {
    {"components", nullptr, nullptr, &Options::components},                 // PREFIX.components.tsv and .components.summary.tsv, the connected components under --overlap-ends' H and F
};

constexpr size_t kLongOptionCount = sizeof(kLongOptions) / sizeof(kLongOptions[0]);
constexpr size_t long_option_count() { return kLongOptionCount + sizeof(kLaterLongOptions) / sizeof(kLaterLongOptions[0]); }
constexpr const LongOption &long_option(size_t k) { return k < kLongOptionCount ? kLongOptions[k] : kLaterLongOptions[k - kLongOptionCount]; }

// Those two are what long_option counts through, and that stays so: 14 rows.  The options behind them stand in a third table, and
// any_long_option(k), k < any_long_option_count(), counts through all three (the command line itself walks kLongOptionTables, below).
inline constexpr LongOption kStringGraphLongOptions[] = {
    {"string-graph", nullptr, nullptr, &Options::string_graph},             // PREFIX.string_graph.gfa and .string_graph.tsv, the transitively reduced dovetails under --overlap-ends' H and F
    {"string-graph-fuzz", parse_string_graph_fuzz, &Options::string_graph_fuzz, &Options::string_graph_fuzz_given},   // Z: how far a path may miss the arc it implies
};

constexpr size_t any_long_option_count() { return long_option_count() + sizeof(kStringGraphLongOptions) / sizeof(kStringGraphLongOptions[0]); }
constexpr const LongOption &any_long_option(size_t k) { return k < long_option_count() ? long_option(k) : kStringGraphLongOptions[k - long_option_count()]; }

// Those three are what any_long_option counts through, and that stays so: 16 rows.  What came behind stands in a fourth table, and the
// command line -- getopt's array, the lookup of a row it found, the check programs -- walks ONE list of tables: the next option is a
// row of the last table, or a table more in the list, and needs no accessor of its own.
inline constexpr LongOption kContainmentLongOptions[] = {
    {"containment", nullptr, nullptr, &Options::containment},               // PREFIX.containment.tsv (with --unitigs also .unitigs.depth.tsv), the forest of the contained reads under --overlap-ends' H and F
};

struct LongOptionTable { const LongOption *rows; size_t count; };
inline constexpr LongOptionTable kLongOptionTables[] = {
    {kLongOptions, sizeof(kLongOptions) / sizeof(kLongOptions[0])},
    {kLaterLongOptions, sizeof(kLaterLongOptions) / sizeof(kLaterLongOptions[0])},
    {kStringGraphLongOptions, sizeof(kStringGraphLongOptions) / sizeof(kStringGraphLongOptions[0])},
    {kContainmentLongOptions, sizeof(kContainmentLongOptions) / sizeof(kContainmentLongOptions[0])},
};

constexpr size_t every_long_option_count()
{
    size_t n = 0;
    for (const LongOptionTable &t : kLongOptionTables) n += t.count;
    return n;
}
// row k of the tables laid end to end, k < every_long_option_count()
constexpr const LongOption &every_long_option(size_t k)
{
    size_t t = 0;
    while (k >= kLongOptionTables[t].count) k -= kLongOptionTables[t++].count;
    return kLongOptionTables[t].rows[k];
}

// Those four tables are what every_long_option counts through, and that stays so: 17 rows.  kOpenLongOptions is the open table: the
// next option is a row here, and nothing counts its rows.  The command line lays it behind the seventeen: getopt's row k is
// every_long_option(k) below every_long_option_count() and kOpenLongOptions[k - every_long_option_count()] from there on.
inline constexpr LongOption kOpenLongOptions[] = {
    {"graph-clean", nullptr, nullptr, &Options::graph_clean},               // PREFIX.clean.tsv, .clean.string_graph.*, .clean.unitigs.*: --string-graph's graph without weak edges and tips
    {"clean-min-ratio", parse_clean_min_ratio, &Options::clean_min_ratio, &Options::clean_min_ratio_given},   // W, in per mille of the end's best span
    {"clean-tip-reads", parse_clean_tip_reads, &Options::clean_tip_reads, &Options::clean_tip_reads_given},   // T: the longest chain that can be a tip
    {"clean-rounds", parse_clean_rounds, &Options::clean_rounds, &Options::clean_rounds_given},               // R: at most that many tip rounds
};
constexpr size_t kOpenLongOptionCount = sizeof(kOpenLongOptions) / sizeof(kOpenLongOptions[0]);

// One long option as getopt found it (text: its argument, NULL for a flag).  false: the text is not what the option takes -- a
// usage error, and the value is left alone.
inline bool set_long_option(const LongOption &o, const char *text, Options *p)
{
    if (o.parse && !o.parse(text, &(p->*o.value))) return false;
    if (o.flag) p->*o.flag = true;
    return true;
}

// The options that mean nothing without another: --ends-min-ratio needs --overlap-ends; --best-overlaps needs it too (it takes its H
// and F from it and its mask from that option's status bytes); --unitigs needs --best-overlaps, whose table it walks;
// --fragment-paf-min needs --fragment-paf; --components needs --overlap-ends, whose H and F it classifies under, and so does
// --string-graph; --string-graph-fuzz needs --string-graph; --containment needs --overlap-ends for the same reason; --graph-clean needs
// --string-graph, whose edge list it takes, and --clean-min-ratio, --clean-tip-reads and --clean-rounds need --graph-clean.
// false: a usage error.
inline bool usage_ok(const Options &o)
{
    return (o.overlap_ends >= 0 || !o.ends_ratio_given) && (!o.best_overlaps || o.overlap_ends >= 0) && (!o.unitigs || o.best_overlaps) &&
           (o.fragment_paf || !o.fragment_paf_min_given) && (!o.components || o.overlap_ends >= 0) &&
           (!o.string_graph || o.overlap_ends >= 0) && (o.string_graph || !o.string_graph_fuzz_given) && (!o.containment || o.overlap_ends >= 0) &&
           (!o.graph_clean || o.string_graph) && (o.graph_clean || !(o.clean_min_ratio_given || o.clean_tip_reads_given || o.clean_rounds_given));
}

// What the options ask of the job between them, decided once (prepare: the group offsets and window records are made by the
// command line, RAFT_CLI_PREPARE on a job without ranks).
struct Request {
    bool filter;                    // --min-identity or --min-overlap: the records are filtered before anything else sees them
    bool strand;                    // the strand byte is tokenised: --overlap-ends and --fragment-paf read it
    bool quality_kept;              // PAF fields 10 and 11 follow the kept records: --fragment-paf writes them beside the filter
    int paf_columns;                // the mask of raft_host_paf_parse_with: fields 10 and 11 for the filter, the strand
    bool keep_query_ids;            // prepare_input writes window records over the query column, which three options read after the job
    bool survey;                    // one one-piece pass before the job: -e auto, --read-stats, --low-cov, --repeat-stats
    bool repeat_stats_second_pass;  // -e auto: the survey ran under a placeholder, the stats pass runs under the estimate
};

inline Request request(const Options &o, bool prepare)
{
    Request r{};
    r.filter = o.min_identity > 0 || o.min_overlap > 0;
    r.strand = o.overlap_ends >= 0 || o.fragment_paf;
    r.quality_kept = r.filter && o.fragment_paf;
    r.paf_columns = (r.filter ? RAFT_HOST_PAF_QUALITY : 0) | (r.strand ? RAFT_HOST_PAF_STRAND : 0);
    r.keep_query_ids = prepare && (o.min_anchor > 0 || o.fragment_overlaps || o.fragment_paf);
    r.survey = o.auto_cov || o.read_stats || o.low_cov >= 0 || o.repeat_stats;
    r.repeat_stats_second_pass = o.auto_cov && o.repeat_stats;
    return r;
}

// ... a read counts as uncovered when more than this many thousandths of its bases lie in low runs (yacrd's default for "not covered")
constexpr int32_t kLowUncoveredPermille = 800;

// The run arrays' first size: real data has a few runs per read (heads, tails, the odd gap); the call says what it needs when
// that is not enough, and never more than RAFT_HIP_LOW_RUNS_MAX.
inline int64_t low_run_capacity0(int64_t n_win, int32_t n_reads)
{
    return std::min<int64_t>(RAFT_HIP_LOW_RUNS_MAX(n_win, n_reads), 4 * (int64_t)n_reads + 1024);
}

// starttime of /proc/self/stat, in clock ticks since boot: field 22, counted behind the LAST ')' (state is field 3), so that a
// command name with blanks or parentheses does not shift the fields.  0: not there.
inline unsigned long long stat_start_time(const char *stat_text)
{
    unsigned long long start = 0;
    if (const char *q = strrchr(stat_text, ')')) {
        int field = 2;
        for (const char *t = q + 1; *t && field < 22; ++t)
            if (*t == ' ') { ++field; if (field == 22) start = strtoull(t + 1, nullptr, 10); }
    }
    return start;
}

// `TIMING devices_used N input ...` and `TIMING coverage_encoding ...`
inline const char *input_label(int ranks, bool windows, int n_runs, bool sym)
{
    return ranks > 0 ? "pre-split slices (one exchange step)"
                     : windows ? "windows" : (n_runs > 0 ? "grouped" : (sym ? "columns (offsets and window records derived by the engine)" : "columns"));
}

inline const char *encoding_label(int cov_width) { return cov_width == RAFT_HIP_COV_DELTA4 ? "delta4" : (cov_width == 2 ? "uint16" : "uint8"); }

} // namespace raft_cli
