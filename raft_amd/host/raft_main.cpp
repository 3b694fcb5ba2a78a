// raft_main.cpp -- `raft [options] <input-reads.fa> <in.paf>`: the reference's command line (main.cpp:21-87,
// chop.hpp:331-373) in front of the MI355X engine.  Host code only tokenises text, resolves names and formats the
// four output files; everything between "records are integers" and "fragment bounds exist" runs on the GPU through
// the C ABI of include/raft_hip.h.  There is no CPU fallback: without libraft_hip.so / a gfx950 device it fails.
//
// Kept on purpose (they change file names or exit codes): -p sets repeat_length AND
// interval_length (main.cpp:44-47); -v falls through into -o (main.cpp:51-55); -i is accepted by getopt but has
// no case, so it prints the usage and exits 1 (main.cpp:56-57); PREFIX.reads.fasta is created before the inputs
// are validated (chop.hpp:333-349); messages go to stdout.
//
// main() is a list of phases over one Job.  What a phase decides from plain values is in cli_plan.hpp; the environment is read
// in read_switches() and nowhere else (but for the exit block of main()).  Four helper threads run beside the main thread:
// bring_up (the device contexts), paf_reader (the bytes of the overlaps file), out_prep (the arrays the results come back in)
// and fasta_writer; where each is joined is part of what a phase does, and die() joins whatever still runs.
#include "../../include/raft_hip.h"
#include "../../include/raft_hip_low.h"
#include "../../include/raft_host_low.h"
#include "../../include/raft_hip_ovl.h"
#include "../../include/raft_host_ovl.h"
#include "../../include/raft_hip_frag.h"
#include "../../include/raft_host_frag.h"
#include "../../include/raft_hip_rst.h"
#include "../../include/raft_host_rst.h"
#include "../../include/raft_hip_flt.h"
#include "../../include/raft_host_flt.h"
#include "../../include/raft_hip_end.h"
#include "../../include/raft_host_end.h"
#include "../../include/raft_hip_best.h"
#include "../../include/raft_host_best.h"
#include "../../include/raft_hip_utg.h"
#include "../../include/raft_host_utg.h"
#include "../../include/raft_hip_lift.h"
#include "../../include/raft_host_lift.h"
#include "../../include/raft_host.h"
#include "cli_plan.hpp"

#include <getopt.h>
#include <unistd.h>

#include <chrono>
#include <thread>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <fstream>
#include <future>
#include <iostream>
#include <ctime>
#include <string>
#include <vector>

namespace {

struct Params {            // param.hpp:18-31
    int reso = 50, est_cov = 0;
    double cov_mul = 1.5;
    int repeat_length = 10000, interval_length = 10000, read_length = 20000, overlap_length = 500, flanking_length = 1000;
    std::string prefix = "raft";
    bool auto_cov = false;         // -e auto: est_cov is read from the data (a survey pass and its coverage histogram) before the job
    bool read_stats = false;       // --read-stats: PREFIX.read_stats.tsv, the per-read table (raft_hip_read_stats, raft_hip_census_host)
    int32_t low_cov = -1;          // --low-cov C: PREFIX.low_coverage.bed, the runs of windows with coverage <= C (raft_hip_low_coverage); -1: not asked for
    bool fragment_overlaps = false;   // --fragment-overlaps: PREFIX.fragments.tsv, the fragments against the overlaps (raft_hip_frag_overlaps_host)
    bool repeat_stats = false;     // --repeat-stats: PREFIX.long_repeats.stats.tsv, one line per repeat run (raft_hip_repeat_stats_host)
    int32_t min_identity = 0;      // --min-identity PCT, in per mille, and --min-overlap BASES: only the records that pass go into the job
    int32_t min_overlap = 0;       // (raft_hip_filter_overlaps_host, before anything else sees the stream); 0: not asked for
    int32_t overlap_ends = -1;     // --overlap-ends H: PREFIX.overlap_ends.tsv, the kind of every record and the ends of every read (raft_hip_overlap_ends_host); -1: not asked for
    int32_t ends_min_ratio = raft_cli::kEndsMinRatioDefault;   // --ends-min-ratio F, in per mille
    bool ends_ratio_given = false;
    bool best_overlaps = false;    // --best-overlaps: PREFIX.best_overlaps.tsv, the best overlap of every read end under --overlap-ends' H and F (raft_hip_best_overlaps_host)
    bool unitigs = false;          // --unitigs: PREFIX.unitigs.tsv and .unitigs.layout.tsv, the chains and cycles of --best-overlaps' mutual ends (raft_hip_unitigs_host)
    int32_t min_anchor = 0;        // --repeat-overlaps A: PREFIX.repeat_overlaps.tsv and .records.tsv (raft_hip_repeat_overlaps_host); 0: not asked for
    bool fragment_paf = false;     // --fragment-paf: PREFIX.fragments.paf, the job's overlaps lifted onto its fragments (raft_hip_lift_overlaps_host)
    int32_t fragment_paf_min = raft_cli::kFragmentPafMinDefault;   // --fragment-paf-min L: pairs shorter than L on either side are dropped
    bool fragment_paf_min_given = false;
};

struct Switches {                  // the environment, as read_switches() found it
    bool timing = false, no_warm_up = false, no_pin = false, no_delta4 = false, cli_prepare = false, no_grouped = false, no_windows = false;
    int context_width = 4;         // the width the first context has outside the survey
    int chunks = 0;                // 0: the engine decides (one piece for small inputs)
};

struct Job {
    Params p;
    const char *reads_fn = nullptr, *paf_fn = nullptr;
    std::string fasta_out;
    raft_hip_params hp{};
    Switches sw;
    std::chrono::system_clock::time_point t_start;              // the reference's timer
    std::chrono::steady_clock::time_point t_main, t_prev;       // the stage clock
    // the devices: context d is on devices[d]; ranks > 0: the pre-split job
    std::vector<int> devices;
    int ranks = 0;
    std::vector<raft_hip_ctx *> ctxs;
    std::vector<int> create_rc;
    std::promise<void> devices_up_p;
    std::shared_future<void> devices_up;
    // the inputs
    raft_host_text *paf_text = nullptr;
    int paf_text_rc = RAFT_HOST_OK;
    raft_host_reads *reads = nullptr;
    int32_t n_reads = 0;
    const int32_t *rl = nullptr;
    raft_host_paf *paf = nullptr;
    int64_t n_rec = 0;
    const int32_t *col[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};    // qid, qs, qe, tid, ts, te
    // --min-identity / --min-overlap: what the filter counted; from then on n_rec, col and the symmetric flag are the kept stream's
    raft_hip_flt_summary flt_sum{};
    bool filtered = false;
    // --overlap-ends: the strand byte of every record (the tokeniser's, or strand_kept for the kept stream), the reads' counts and status
    const uint8_t *strand = nullptr;
    std::vector<uint8_t> strand_kept, end_status;
    std::vector<int32_t> end_counts;
    raft_hip_end_summary end_sum{};
    // --best-overlaps: per read end the partner and the span, per read the flag byte
    std::vector<int32_t> best_partner, best_span;
    std::vector<uint8_t> best_flags;
    raft_hip_best_summary best_sum{};
    // --unitigs: per read the unitig, the place in it, the offset and the orientation; the layout order; per unitig size, length, circular
    std::vector<int32_t> utg_unitig, utg_index, utg_order, utg_reads;
    std::vector<int64_t> utg_offset, utg_off, utg_length;
    std::vector<uint8_t> utg_orient, utg_circular;
    raft_hip_utg_summary utg_sum{};
    // --fragment-paf: the eight columns of the lifted stream; PAF fields 10 and 11 of the kept records where the filter tokenised them
    std::vector<int32_t> lift_col[6], lift_src, matches_kept, block_kept;
    std::vector<uint8_t> lift_rev;
    const int32_t *lift_matches = nullptr, *lift_block = nullptr;
    raft_hip_lift_summary lift_sum{};
    // the arrays everything comes back in (made and page-locked on out_prep)
    raft_cli::Capacities cap;
    std::vector<int64_t> cov_off, rep_off, frag_off;
    std::unique_ptr<uint8_t[]> cov8;
    int64_t cov8_locked = 0;                  // the bytes of cov8 that are page-locked (cli_plan.hpp cov_bytes_needed)
    std::unique_ptr<int32_t[]> rep_s, rep_e, fb, fe;
    std::vector<int64_t> exc_i;
    std::vector<int32_t> exc_v;
    std::vector<int32_t> cov_anchor;          // the four-bit step encoding's block anchors (cov_width = RAFT_HIP_COV_DELTA4)
    // --read-stats: the survey's coverage summary and the census of the record stream
    std::vector<int64_t> rs_sum;
    std::vector<int32_t> rs_max, rs_high, cen_intervals;
    std::vector<uint8_t> cen_contained;
    int64_t n_contained = 0;
    // --low-cov: the survey's low-coverage runs
    std::vector<int64_t> low_off;
    std::vector<int32_t> low_s, low_e;
    raft_hip_low_summary low_sum{};
    // --repeat-overlaps: the records' class bytes, the reads' tallies and flags; the query column as tokenised where prepare_input writes over it
    std::vector<uint8_t> ovl_cls, ovl_flags;
    std::vector<int32_t> ovl_touch, ovl_repeat, ovl_qid;
    raft_hip_ovl_summary ovl_sum{};
    // --fragment-overlaps: per fragment the sides that touch, span and contain it, its bases inside repeats
    std::vector<int32_t> frag_touch, frag_span, frag_contained, frag_repeat;
    raft_hip_frag_summary frag_sum{};
    // --repeat-stats: per repeat run of the stats pass the sides that touch, span and lie inside it, its coverage, its flags
    std::vector<int32_t> rst_touch, rst_span, rst_inside, rst_windows, rst_min, rst_max, rst_high;
    std::vector<int64_t> rst_cov_sum;
    std::vector<uint8_t> rst_flags;
    raft_hip_rst_summary rst_sum{};
    bool rst_done = false;
    // the form the job is handed over in, and what it brought back
    std::unique_ptr<int64_t[]> rec_off;
    int32_t n_runs = 0;
    const uint32_t *win = nullptr;
    bool sym = false;
    int cov_width = 1;
    raft_hip_summary s{};
    int64_t n_exc = 0;
    int n_attempts = 0;                       // engine calls of the ladder (run_engine)
    int fasta_rc = RAFT_HOST_OK;
    std::thread bring_up, paf_reader, out_prep, fasta_writer;
};

Job *g_job = nullptr;      // for die()

[[noreturn]] void print_help(const Params &p) // main.cpp:7-19
{
    std::cout << "Usage: raft [options] <input-reads.fa> <in.paf>\n";
    std::cout << "  -r NUM     resolution of coverage " << p.reso << "\n";
    std::cout << "  -e NUM     estimated coverage " << "\n";
    std::cout << "  -m NUM     coverage multiplier " << p.cov_mul << "\n";
    std::cout << "  -l NUM     read_length " << p.read_length << "\n";
    std::cout << "  -v NUM     overlap_length " << p.overlap_length << "\n";
    std::cout << "  -p NUM     repeat_length " << p.repeat_length << "\n";
    std::cout << "  -f NUM     flanking_length " << p.flanking_length << "\n";
    std::cout << "  -o FILE    prefix of output files " << p.prefix << "\n";
    std::cout.flush();
    exit(1);
}

bool missing_or_empty(const char *fn) // chop.hpp:326-329,336-349
{
    std::ifstream f(fn);
    return !f || f.peek() == std::ifstream::traits_type::eof();
}

// Main thread only.  The helpers must be finished before the process exits.
[[noreturn]] void die(const std::string &msg)
{
    if (g_job)
        for (std::thread *t : {&g_job->bring_up, &g_job->fasta_writer, &g_job->paf_reader, &g_job->out_prep})
            if (t->joinable()) t->join();
    std::cout << msg << "\n";
    std::cout.flush();
    exit(1);
}

std::string engine_error(const Job &j, int code, int64_t index)
{
    std::string m = std::string("ERROR, raft_hip, ") + raft_hip_strerror(code);
    if (index >= 0) m += " (index " + std::to_string(index) + ")";
    const char *d = raft_hip_last_error(j.ctxs[0]);
    if (d && *d) m += std::string(" [") + d + "]";
    return m;
}

// stage clock on stderr when RAFT_TIMING is set (stdout stays the reference's)
void stage(Job &j, const char *what)
{
    const auto now = std::chrono::steady_clock::now();
    if (j.sw.timing) fprintf(stderr, "TIMING %-16s %8.3f s\n", what, std::chrono::duration<double>(now - j.t_prev).count());
    j.t_prev = now;
}

// Arrays that cross PCIe are page-locked once the runtime is up (raft_hip_host_register: the link's 53 GB/s instead of
// the runtime's staging of pageable memory); not worth the calls for small inputs.  A failed registration is not an
// error: the copy then takes the pageable path.
void pin(const Job &j, const void *ptr, size_t bytes)
{
    if (!j.sw.no_pin && ptr && bytes >= (size_t)(64u << 10)) (void)raft_hip_host_register(const_cast<void *>(ptr), bytes);
}

void parse_options(Job &j, int argc, char *argv[])
{
    Params &p = j.p;
    int option;
    // (the short options and their quirks are the reference's; the long options are this program's own)
    static const struct option long_options[] = {{"read-stats", no_argument, nullptr, 1000}, {"low-cov", required_argument, nullptr, 1001},
                                                 {"repeat-overlaps", required_argument, nullptr, 1002}, {"fragment-overlaps", no_argument, nullptr, 1003},
                                                 {"repeat-stats", no_argument, nullptr, 1004}, {"min-identity", required_argument, nullptr, 1005},
                                                 {"min-overlap", required_argument, nullptr, 1006},
                                                 {"overlap-ends", required_argument, nullptr, 1007}, {"ends-min-ratio", required_argument, nullptr, 1008},
                                                 {"best-overlaps", no_argument, nullptr, 1009}, {"unitigs", no_argument, nullptr, 1010},
                                                 {"fragment-paf", no_argument, nullptr, 1011}, {"fragment-paf-min", required_argument, nullptr, 1012},
                                                 {nullptr, 0, nullptr, 0}};
    while ((option = getopt_long(argc, argv, "r:e:m:l:i:p:f:v:o:", long_options, nullptr)) != -1) {
        switch (option) {
        case 1000: p.read_stats = true; break;
        case 1001: if (!raft_cli::parse_low_cov(optarg, &p.low_cov)) print_help(p); break;
        case 1002: if (!raft_cli::parse_min_anchor(optarg, &p.min_anchor)) print_help(p); break;
        case 1003: p.fragment_overlaps = true; break;
        case 1004: p.repeat_stats = true; break;
        case 1005: if (!raft_cli::parse_min_identity(optarg, &p.min_identity)) print_help(p); break;
        case 1006: if (!raft_cli::parse_min_overlap(optarg, &p.min_overlap)) print_help(p); break;
        case 1007: if (!raft_cli::parse_overlap_ends(optarg, &p.overlap_ends)) print_help(p); break;
        case 1008: if (!raft_cli::parse_ends_min_ratio(optarg, &p.ends_min_ratio)) print_help(p); p.ends_ratio_given = true; break;
        case 1009: p.best_overlaps = true; break;
        case 1010: p.unitigs = true; break;
        case 1011: p.fragment_paf = true; break;
        case 1012: if (!raft_cli::parse_fragment_paf_min(optarg, &p.fragment_paf_min)) print_help(p); p.fragment_paf_min_given = true; break;
        case 'r': p.reso = atoi(optarg); break;
        case 'e': p.auto_cov = strcmp(optarg, "auto") == 0; p.est_cov = p.auto_cov ? 0 : atoi(optarg); break;
        case 'm': p.cov_mul = std::stod(optarg); break;
        case 'l': p.read_length = atoi(optarg); break;
        case 'p': p.repeat_length = atoi(optarg); p.interval_length = atoi(optarg); break;
        case 'f': p.flanking_length = atoi(optarg); break;
        case 'v': p.overlap_length = atoi(optarg); // no break in the reference: -v also sets the prefix (main.cpp:51-55)
                  /* fall through */
        case 'o': p.prefix = optarg; break;
        default: print_help(p);
        }
    }
    if (!raft_cli::ends_options_ok(p.overlap_ends, p.ends_ratio_given)) print_help(p);
    if (!raft_cli::best_options_ok(p.best_overlaps, p.overlap_ends)) print_help(p);
    if (!raft_cli::unitigs_options_ok(p.unitigs, p.best_overlaps)) print_help(p);
    if (!raft_cli::fragment_paf_options_ok(p.fragment_paf, p.fragment_paf_min_given)) print_help(p);
    if (argc < optind + 2) print_help(p);
    if (p.est_cov <= 0 && !p.auto_cov) {
        std::cout << "ERROR, main(), estimated coverage must be set properly\n";
        print_help(p);
    }
    j.reads_fn = argv[optind];
    j.paf_fn = argv[optind + 1];
    j.fasta_out = p.prefix + ".reads.fasta";
}

void print_params(Job &j) // param.hpp:33-43, and main.cpp's timer
{
    const Params &p = j.p;
    std::cout << "INFO, printParams(), reso = " << p.reso << "\n";
    if (p.auto_cov) std::cout << "INFO, printParams(), est_cov = auto\n";
    else std::cout << "INFO, printParams(), est_cov = " << p.est_cov << "\n";
    std::cout << "INFO, printParams(), cov_mul = " << p.cov_mul << "\n";
    std::cout << "INFO, printParams(), repeat_length = " << p.repeat_length << "\n";
    std::cout << "INFO, printParams(), interval_length = " << p.interval_length << "\n";
    std::cout << "INFO, printParams(), read_length = " << p.read_length << "\n";
    std::cout << "INFO, printParams(), overlap_length = " << p.overlap_length << "\n";
    std::cout << "INFO, printParams(), flanking_length = " << p.flanking_length << "\n";

    j.t_start = std::chrono::system_clock::now();
    std::cout << "INFO, main(), started timer\n";
}

void check_inputs(Job &j)
{
    { std::ofstream touch(j.fasta_out); }               // chop.hpp:333: created before any validation
    if (missing_or_empty(j.reads_fn)) die(std::string("ERROR, break_long_reads(), ") + j.reads_fn + " input file either does not exist or is empty");
    if (missing_or_empty(j.paf_fn)) die(std::string("ERROR, break_long_reads(), ") + j.paf_fn + " input file either does not exist or is empty");
}

// what the contexts are created under; symmetric_mode follows once the overlaps are tokenised (hand_over_symmetric_flag)
void fill_engine_params(Job &j)
{
    const Params &p = j.p;
    raft_hip_params &hp = j.hp;
    hp.reso = p.reso; hp.est_cov = p.auto_cov ? 1 : p.est_cov;   // (-e auto: a placeholder until the survey -- create rejects 0)
    hp.cov_mul = p.cov_mul; hp.repeat_length = p.repeat_length;
    hp.interval_length = p.interval_length; hp.read_length = p.read_length; hp.overlap_length = p.overlap_length;
    hp.flanking_length = p.flanking_length; hp.symmetric_mode = -1;
}

// The one place that reads the environment (the exit block of main() apart).
void read_switches(Job &j)
{
    Switches &sw = j.sw;
    sw.timing = getenv("RAFT_TIMING") != nullptr;              // the stage clock on stderr
    // which devices share the job, and whether it is the pre-split job of N ranks (cli_plan.hpp device_list)
    const raft_cli::DeviceList l = raft_cli::device_list(getenv("RAFT_DEVICES"), getenv("RAFT_DEVICE"), getenv("RAFT_RANKS"));
    j.devices = l.devices;
    j.ranks = l.ranks;
    sw.no_warm_up = getenv("RAFT_NO_WARM_UP") != nullptr;      // contexts are not warmed up, device buffers not reserved ahead of the job
    sw.no_pin = getenv("RAFT_NO_PIN") != nullptr;              // host arrays stay pageable
    sw.no_delta4 = getenv("RAFT_NO_DELTA4") != nullptr;        // coverage comes back in a byte encoding whatever the input's shape
    sw.context_width = raft_cli::context_cov_width(getenv("RAFT_COV_WIDTH"));   // read by the engine at create: what the survey puts back
    sw.cli_prepare = getenv("RAFT_CLI_PREPARE") != nullptr;    // group offsets and window records are made here, not by the engine
    sw.no_grouped = getenv("RAFT_NO_GROUPED") != nullptr;      // ... but no group offsets: the plain columns go up
    sw.no_windows = getenv("RAFT_NO_WINDOWS") != nullptr;      // ... but no window records: the coordinate columns go up
    const char *chunks = getenv("RAFT_CHUNKS");                // pieces of the chunked pipeline; 0 / unset: the engine decides
    sw.chunks = chunks ? atoi(chunks) : 0;
}

// What the stage clock cannot see from inside (1.4 s of a 4.8 s run appeared in no stage): how old the process was
// when main() got here -- the loader mapping libamdhip64 and friends -- and, at the end, the moment main() leaves, so that
// whoever started the process can tell what the teardown behind _exit took (tools/cli_big.py prints both).  -1: not known.
double process_age()
{
    FILE *f = fopen("/proc/self/stat", "r");
    if (!f) return -1.0;
    char buf[1024];
    const size_t n = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[n] = 0;
    const unsigned long long start = raft_cli::stat_start_time(buf);
    if (!start) return -1.0;
    double up = 0.0;
    if (FILE *u = fopen("/proc/uptime", "r")) { if (fscanf(u, "%lf", &up) != 1) up = 0.0; fclose(u); }
    return up > 0.0 ? up - (double)start / (double)sysconf(_SC_CLK_TCK) : -1.0;
}

void start_clock(Job &j)
{
    j.t_prev = std::chrono::steady_clock::now();
    j.t_main = j.t_prev;
    if (j.sw.timing) fprintf(stderr, "TIMING %-16s %8.3f s\n", "process->main", process_age());
}

// The device contexts come up (runtime init, first allocations) while the host tokenises the inputs: created and warmed up --
// the engine's code goes to the device, the pipeline's lanes come up: 70-80 ms that would otherwise sit inside the first job.
// j.hp is read by these threads: nobody writes it before bring_up is joined.
void start_devices(Job &j)
{
    j.ctxs.assign(j.devices.size(), nullptr);
    j.create_rc.assign(j.devices.size(), RAFT_HIP_OK);
    j.devices_up = j.devices_up_p.get_future().share();
    j.bring_up = std::thread([&j] {
        std::vector<std::thread> th;
        auto up = [&j](size_t d) {
            j.create_rc[d] = raft_hip_create(j.devices[d], &j.hp, &j.ctxs[d]);
            if (j.create_rc[d] == RAFT_HIP_OK && !j.sw.no_warm_up) j.create_rc[d] = raft_hip_warm_up(j.ctxs[d]);
        };
        for (size_t d = 1; d < j.devices.size(); ++d) th.emplace_back([&up, d] { up(d); });
        up(0);
        for (auto &t : th) t.join();
        j.devices_up_p.set_value();
    });
}

// The overlaps file's bytes need nothing of the reads: they are read -- inflated, for a .gz -- beside the loading of
// the reads (on gz inputs, the reference's own quick-start shape, the two inflations are most of the run).
void start_paf_read(Job &j)
{
    j.paf_reader = std::thread([&j] { j.paf_text_rc = raft_host_text_read(j.paf_fn, &j.paf_text); });
}

void load_reads(Job &j)
{
    const int rc = raft_host_reads_load(j.reads_fn, &j.reads);
    stage(j, "reads_load");
    if (rc == RAFT_HOST_ERR_DUP_NAME) die("ERROR, loadFASTA(), two reads share a name");
    if (rc != RAFT_HOST_OK) die(std::string("ERROR, loadFASTA(), cannot read ") + j.reads_fn);
    j.n_reads = raft_host_reads_count(j.reads);
    j.rl = raft_host_reads_lengths(j.reads);
    std::cout.flush();
    if (j.n_reads > 0) fprintf(stdout, "Real Reads %d \n", raft_host_reads_real(j.reads)); // chop.hpp:105
}

// On out_prep.  Host arrays for everything that comes back, sized by the bounds of raft_hip.h (from the read lengths alone).
// Coverage returns in its transfer encoding (a byte per window + the windows at or above 255): a quarter of the
// int32 array's bytes over PCIe, and the formatter reads it as it is.  They are allocated and page-locked beside
// the tokenising of the overlaps (pinning untouched pages costs their first touch: 0.1 s for the 2 GB of a human set);
// page-locking and reserving wait for the contexts and are left out when one of them did not come up.  The coverage array is
// page-locked for the byte width of the first attempt; an attempt of the ladder that needs more registers it anew (run_engine).
void prepare_outputs(Job &j)
{
    const Params &p = j.p;
    j.cap = raft_cli::output_capacities(j.n_reads, j.rl, p.reso, p.repeat_length, p.interval_length);
    const raft_cli::Capacities &c = j.cap;
    j.cov8.reset(new uint8_t[(size_t)c.cov8_bytes]);                              // (not value-initialised: no zero fill)
    j.rep_s.reset(new int32_t[(size_t)c.rep_cap + 1]); j.rep_e.reset(new int32_t[(size_t)c.rep_cap + 1]);
    j.fb.reset(new int32_t[(size_t)c.frag_cap + 1]); j.fe.reset(new int32_t[(size_t)c.frag_cap + 1]);
    j.exc_i.resize((size_t)c.exc_cap0); j.exc_v.resize((size_t)c.exc_cap0);
    j.cov_anchor.resize((size_t)c.n_anchor);
    j.devices_up.wait();
    for (size_t d = 0; d < j.devices.size(); ++d) if (j.create_rc[d] != RAFT_HIP_OK) return;
    pin(j, j.exc_i.data(), j.exc_i.size() * 8); pin(j, j.exc_v.data(), j.exc_v.size() * 4);
    pin(j, j.cov_anchor.data(), j.cov_anchor.size() * 4);
    j.cov8_locked = raft_cli::cov_bytes_needed(raft_cli::byte_width(p.auto_cov, p.est_cov), c.n_win);
    pin(j, j.cov8.get(), (size_t)j.cov8_locked);
    pin(j, j.fb.get(), ((size_t)c.frag_cap + 1) * 4); pin(j, j.fe.get(), ((size_t)c.frag_cap + 1) * 4);
    pin(j, j.rep_s.get(), ((size_t)c.rep_cap + 1) * 4); pin(j, j.rep_e.get(), ((size_t)c.rep_cap + 1) * 4);
    pin(j, j.cov_off.data(), j.cov_off.size() * 8); pin(j, j.frag_off.data(), j.frag_off.size() * 8); pin(j, j.rep_off.data(), j.rep_off.size() * 8);
    pin(j, j.rl, (size_t)j.n_reads * 4);
    // the job's device buffers, sized from what is known by now: the reads' lengths, and the record count from the size of the
    // overlaps file (cli_plan.hpp record_estimate)
    if (!j.sw.no_warm_up) {
        std::ifstream pf(j.paf_fn, std::ios::binary | std::ios::ate);
        const int64_t est = pf ? raft_cli::record_estimate((int64_t)pf.tellg(), j.paf_fn) : 0;
        for (size_t d = 0; d < j.devices.size(); ++d)
            (void)raft_hip_reserve(j.ctxs[d], j.n_reads, j.rl, est, (int32_t)j.devices.size(), raft_cli::reserve_cov_width(j.sw.no_delta4, p.auto_cov, p.est_cov));
    }
}

void start_output_prep(Job &j)
{
    j.cov_off.resize((size_t)j.n_reads + 1); j.rep_off.resize((size_t)j.n_reads + 1); j.frag_off.resize((size_t)j.n_reads + 1);
    j.out_prep = std::thread([&j] { prepare_outputs(j); });
}

void parse_paf(Job &j)
{
    char bad[256] = {0};
    j.paf_reader.join();
    stage(j, "paf_read (rest)");
    int rc = j.paf_text_rc;
    // (the filter reads PAF columns 10 and 11, --overlap-ends and --fragment-paf the strand; none of them: the plain parser)
    const int columns = raft_cli::paf_columns_with_lift(raft_cli::filter_wanted(j.p.min_identity, j.p.min_overlap), j.p.overlap_ends, j.p.fragment_paf);
    if (rc == RAFT_HOST_OK) rc = raft_host_paf_parse_with(j.paf_text, j.reads, columns, &j.paf, bad, sizeof bad);
    // (a big file's GBs of touched pages are left to the process exit: unmapping them here -- or beside the pass, where it holds
    // the address space's lock against the page-locking -- cost 0.3 s of a 4 s run)
    if (raft_host_paf_count(j.paf) < (1 << 22)) { raft_host_text_free(j.paf_text); j.paf_text = nullptr; }
    if (rc == RAFT_HOST_ERR_UNKNOWN_NAME) die(std::string("ERROR, create_pileup(), read ") + bad + " of the overlaps file is not in the reads file");
    if (rc != RAFT_HOST_OK) die(std::string("ERROR, create_pileup(), cannot read ") + j.paf_fn);
    j.n_rec = raft_host_paf_count(j.paf);
    for (int k = 0; k < 6; ++k) j.col[k] = raft_host_paf_column(j.paf, k);
    j.strand = raft_host_paf_strand(j.paf);
    stage(j, "paf_load");
}

void await_devices(Job &j)
{
    j.bring_up.join();
    for (size_t d = 0; d < j.devices.size(); ++d)
        if (j.create_rc[d] != RAFT_HIP_OK)
            die(std::string("ERROR, raft_hip_create(), device ") + std::to_string(j.devices[d]) + ": " + raft_hip_strerror(j.create_rc[d]));
    stage(j, "device_wait");
}

// --overlap-ends beside the filter: the strand must follow the kept records.  The filter copies its id columns without using them as
// indices (include/raft_hip_flt.h), so one more call of its host form under the same P and L, with the strand bytes widened to int32
// in the query-id slot, compacts them; what it writes for the other five columns is dropped.
void keep_strand(Job &j)
{
    std::vector<int32_t> wide(j.strand, j.strand + j.n_rec), drop[5];
    for (auto &d : drop) d.resize((size_t)j.n_rec);
    raft_hip_flt_summary sum{};
    const int rc = raft_hip_filter_overlaps_host(j.ctxs[0], j.n_rec, wide.data(), j.col[1], j.col[2], j.col[3], j.col[4], j.col[5],
                                                 raft_host_paf_quality(j.paf, 0), raft_host_paf_quality(j.paf, 1), j.p.min_identity, j.p.min_overlap,
                                                 wide.data(), drop[0].data(), drop[1].data(), drop[2].data(), drop[3].data(), drop[4].data(), &sum, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, -1));
    j.strand_kept.assign(wide.begin(), wide.begin() + sum.n_kept);
    j.strand = j.strand_kept.data();
}

// --fragment-paf beside the filter: PAF fields 10 and 11 of the kept records, for the writer, by the same means -- matches in the
// query-id slot, block in the target-id slot.
void keep_quality(Job &j)
{
    const int32_t *m = raft_host_paf_quality(j.paf, 0), *b = raft_host_paf_quality(j.paf, 1);
    j.matches_kept.assign(m, m + j.n_rec); j.block_kept.assign(b, b + j.n_rec);
    std::vector<int32_t> drop[4];
    for (auto &d : drop) d.resize((size_t)j.n_rec);
    raft_hip_flt_summary sum{};
    const int rc = raft_hip_filter_overlaps_host(j.ctxs[0], j.n_rec, j.matches_kept.data(), j.col[1], j.col[2], j.block_kept.data(), j.col[4], j.col[5], m, b,
                                                 j.p.min_identity, j.p.min_overlap, j.matches_kept.data(), drop[0].data(), drop[1].data(),
                                                 j.block_kept.data(), drop[2].data(), drop[3].data(), &sum, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, -1));
    j.matches_kept.resize((size_t)sum.n_kept); j.block_kept.resize((size_t)sum.n_kept);
    j.lift_matches = j.matches_kept.data(); j.lift_block = j.block_kept.data();
}

// --min-identity / --min-overlap: the records that pass (include/raft_hip_flt.h) are compacted in place, on the first context, before
// anything else sees the stream -- the survey, the census, the split of a multi-device or pre-split job, every query: the job is the
// job on a file of the kept lines.  Without the options nothing happens here.
void filter_overlaps(Job &j)
{
    if (!raft_cli::filter_wanted(j.p.min_identity, j.p.min_overlap)) return;
    j.out_prep.join();                                  // (its raft_hip_reserve uses the context this call runs on)
    int32_t *out[6];
    for (int k = 0; k < 6; ++k) out[k] = const_cast<int32_t *>(j.col[k]);
    if (raft_cli::strand_wanted(j.p.overlap_ends, j.p.fragment_paf)) keep_strand(j);   // (first: it reads the columns as tokenised)
    if (j.p.fragment_paf) keep_quality(j);
    const int rc = raft_hip_filter_overlaps_host(j.ctxs[0], j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.col[4], j.col[5],
                                                 raft_host_paf_quality(j.paf, 0), raft_host_paf_quality(j.paf, 1), j.p.min_identity, j.p.min_overlap,
                                                 out[0], out[1], out[2], out[3], out[4], out[5], &j.flt_sum, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, -1));
    j.n_rec = j.flt_sum.n_kept;
    j.filtered = true;
    stage(j, "filter_overlaps");
}

// the symmetric flag of the stream the job runs on: the tokeniser's, or the filter's for the kept stream
bool stream_symmetric(const Job &j) { return j.filtered ? j.flt_sum.symmetric != 0 : raft_host_paf_symmetric(j.paf) != 0; }

// The tokeniser already knows whether the PAF is symmetric (chop.hpp:171-184, found while the lines were in
// registers): the engine is told, so it neither scans for the mirror of record 0 nor -- for a symmetric PAF -- is
// handed the target columns at all (half of the upload).  bring_up is joined: j.hp may be written.
void hand_over_symmetric_flag(Job &j)
{
    j.hp.symmetric_mode = j.ranks > 0 ? -1 : (stream_symmetric(j) ? 1 : 0);   // (a pre-split job finds the flag across its ranks)
    if (j.out_prep.joinable()) j.out_prep.join();       // (its raft_hip_reserve reads the contexts' parameters: done before they change)
    const int rc = raft_hip_set_params(j.ctxs[0], &j.hp);
    if (rc != RAFT_HIP_OK) die(std::string("ERROR, raft_hip_set_params(), ") + raft_hip_strerror(rc));
    j.sym = j.hp.symmetric_mode == 1 || (j.ranks > 0 && stream_symmetric(j));
}

// What the survey changes on the first context, and the way back: its own parameters, two-byte codes and no cut points for the
// pass; then the width the context had and the cut points again (restore_outputs), and the job's parameters (restore_params).
// Both restores are calls whose codes the survey reports.
struct SurveySettings {
    raft_hip_ctx *ctx;
    int width_before;
    int apply(const raft_hip_params &sp)
    {
        int rc = raft_hip_set_params(ctx, &sp);
        if (rc == RAFT_HIP_OK) rc = raft_hip_set_output_width(ctx, 2);
        if (rc == RAFT_HIP_OK) rc = raft_hip_set_emit_cuts(ctx, 0);
        return rc;
    }
    int restore_outputs()
    {
        const int rc = raft_hip_set_output_width(ctx, width_before);
        return rc == RAFT_HIP_OK ? raft_hip_set_emit_cuts(ctx, 1) : rc;
    }
    int restore_params(const raft_hip_params &hp) { return raft_hip_set_params(ctx, &hp); }   // (the first context's parameters are what every device and rank runs under)
};

// --read-stats: the coverage summary of the pass that has just run, under threshold = (int)(est_cov * cov_mul)
int survey_read_stats(Job &j, int est_cov)
{
    j.rs_sum.resize((size_t)j.n_reads); j.rs_max.resize((size_t)j.n_reads); j.rs_high.resize((size_t)j.n_reads);
    const int32_t high_cov = (int32_t)(est_cov * j.p.cov_mul);          // (the job's: repeat.hpp:89-90)
    const int rc = raft_hip_read_stats(j.ctxs[0], std::max(high_cov, 1), j.rs_sum.data(), j.rs_max.data(), j.rs_high.data(), nullptr);
    if (high_cov < 1)                                                    // (every window is at or above a threshold below 1)
        for (int32_t i = 0; i < j.n_reads; ++i) j.rs_high[(size_t)i] = (int32_t)(((int64_t)j.rl[i] + j.p.reso - 1) / j.p.reso);
    return rc;
}

// --low-cov: the low-coverage runs of the pass that has just run.  The run arrays start at cli_plan.hpp's first size; a set with more
// runs says so (RAFT_HIP_ERR_TOO_LARGE and the number) and is asked once more.
int survey_low_coverage(Job &j, int64_t n_win)
{
    j.low_off.resize((size_t)j.n_reads + 1);
    int64_t cap = raft_cli::low_run_capacity0(n_win, j.n_reads);
    int rc = RAFT_HIP_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        j.low_s.resize((size_t)cap); j.low_e.resize((size_t)cap);
        rc = raft_hip_low_coverage(j.ctxs[0], j.p.low_cov, raft_cli::kLowUncoveredPermille, cap, j.low_off.data(), j.low_s.data(), j.low_e.data(), nullptr,
                                   nullptr, &j.low_sum, nullptr);
        if (rc != RAFT_HIP_ERR_TOO_LARGE) break;
        cap = j.low_sum.n_runs;
    }
    return rc;
}

// --repeat-stats: one row per repeat run of the pass that has just run -- its own annotation, its coverage, the tokenised columns
// under the job's symmetric flag as census() hands them over --, before prepare_input() writes window records over the query column.
int survey_repeat_stats(Job &j, int est_cov, int64_t n_repeats, int64_t *bad_index)
{
    for (std::vector<int32_t> *v : {&j.rst_touch, &j.rst_span, &j.rst_inside, &j.rst_windows, &j.rst_min, &j.rst_max, &j.rst_high}) v->resize((size_t)n_repeats);
    j.rst_cov_sum.resize((size_t)n_repeats); j.rst_flags.resize((size_t)n_repeats);
    const raft_hip_records rec{j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.sym ? nullptr : j.col[4], j.sym ? nullptr : j.col[5]};
    j.rst_done = true;
    return raft_hip_repeat_stats_host(j.ctxs[0], j.n_reads, j.rl, &rec, j.sym ? 1 : 0, -1, nullptr, nullptr, nullptr,
                                      raft_cli::repeat_stats_threshold(est_cov, j.p.cov_mul), j.rst_touch.data(), j.rst_span.data(), j.rst_inside.data(),
                                      j.rst_windows.data(), j.rst_min.data(), j.rst_max.data(), j.rst_high.data(), j.rst_cov_sum.data(), j.rst_flags.data(),
                                      &j.rst_sum, bad_index, nullptr);
}

// -e auto: the survey.  cov[] does not depend on est_cov, so one one-piece pass on the first context under the placeholder holds
// the number -e stands for: its coverage histogram is made on the device (32 KiB come back instead of cov[]) and the estimate
// read from it (raft_hip.h).  The pass writes two-byte codes and no cut points -- nothing of it is fetched --, and its
// overlap_length is 0: which fragments there are depends on the repeats, hence on the placeholder, and RAFT_HIP_ERR_FRAGMENT of
// the survey would not be the job's.  Every other data error (ids, coordinates, lengths) is the one the job would report, in
// its words.  With several devices or ranks the survey still runs in one piece on the first: one more upload of the columns.
//
// --read-stats: the per-read table.  Its coverage summary (raft_hip_read_stats) is taken from the same survey pass, right behind
// the histogram; without -e auto one such pass -- the survey's recipe -- runs here for it.  The job itself runs as it does
// without the option.  --low-cov: the same, for the low-coverage runs (raft_hip_low_coverage), behind the two.
// --repeat-stats: the table of the repeat runs (raft_hip_repeat_stats_host) needs coverage AND annotation under the job's final est_cov:
// with -e N the survey pass is that pass; with -e auto one more pass of the same recipe runs under the estimate (one more upload of
// the columns), and the table is taken right behind it.
void survey(Job &j)
{
    Params &p = j.p;
    if (!raft_cli::survey_needed(p.auto_cov, p.read_stats, p.low_cov, p.repeat_stats)) return;
    raft_hip_ctx *ctx = j.ctxs[0];
    SurveySettings settings{ctx, j.sw.context_width};
    raft_hip_params sp = j.hp;
    sp.overlap_length = 0;
    const bool targets = j.hp.symmetric_mode != 1;
    raft_hip_summary ss{};
    ss.error_index = -1;
    int rc = settings.apply(sp);
    if (rc == RAFT_HIP_OK)
        rc = raft_hip_run_host(ctx, j.n_reads, j.rl, j.n_rec, j.col[0], j.col[1], j.col[2], targets ? j.col[3] : nullptr, targets ? j.col[4] : nullptr,
                               targets ? j.col[5] : nullptr);
    if (rc == RAFT_HIP_OK) rc = raft_hip_finish(ctx, &ss);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, ss.error_index));
    raft_hip_cov_estimate est{};
    est.est_cov = p.est_cov;
    if (p.auto_cov) {
        std::vector<int64_t> hist(RAFT_HIP_COV_HIST_BINS);
        rc = raft_hip_cov_histogram(ctx, hist.data(), nullptr);
        if (rc == RAFT_HIP_OK) rc = raft_hip_estimate_coverage(hist.data(), RAFT_HIP_COV_HIST_BINS, &est);
    }
    if (rc == RAFT_HIP_OK && p.read_stats && est.est_cov > 0) rc = survey_read_stats(j, est.est_cov);
    if (rc == RAFT_HIP_OK && p.low_cov >= 0) rc = survey_low_coverage(j, ss.n_bins);
    if (rc == RAFT_HIP_OK && p.repeat_stats && est.est_cov > 0) {
        if (raft_cli::repeat_stats_second_pass(p.auto_cov, p.repeat_stats)) {
            sp.est_cov = est.est_cov;
            rc = raft_hip_set_params(ctx, &sp);
            if (rc == RAFT_HIP_OK)
                rc = raft_hip_run_host(ctx, j.n_reads, j.rl, j.n_rec, j.col[0], j.col[1], j.col[2], targets ? j.col[3] : nullptr, targets ? j.col[4] : nullptr,
                                       targets ? j.col[5] : nullptr);
            if (rc == RAFT_HIP_OK) rc = raft_hip_finish(ctx, &ss);
            if (rc != RAFT_HIP_OK) die(engine_error(j, rc, ss.error_index));
        }
        int64_t bad_index = -1;
        rc = survey_repeat_stats(j, est.est_cov, ss.n_repeats, &bad_index);
        if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    }
    if (rc == RAFT_HIP_OK) rc = settings.restore_outputs();
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, -1));
    stage(j, "estimate");
    if (p.auto_cov) {
        if (est.est_cov <= 0) {                              // no window anybody overlaps: as for -e 0
            std::cout << "ERROR, main(), estimated coverage must be set properly\n";
            print_help(p);
        }
        fprintf(stdout, "INFO, estimate_coverage(), est_cov = %d\n", est.est_cov);
        p.est_cov = est.est_cov;
        j.hp.est_cov = est.est_cov;
    }
    rc = settings.restore_params(j.hp);
    if (rc != RAFT_HIP_OK) die(std::string("ERROR, raft_hip_set_params(), ") + raft_hip_strerror(rc));
}

// --read-stats: the census of the record stream (raft_hip_census_host) reads the tokenised columns under the job's symmetric
// flag, before prepare_input() writes window records over the query column.
void census(Job &j)
{
    if (!j.p.read_stats) return;
    j.cen_intervals.resize((size_t)j.n_reads); j.cen_contained.resize((size_t)j.n_reads);
    int64_t bad_index = -1;
    const int rc = raft_hip_census_host(j.ctxs[0], j.n_reads, j.rl, j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.sym ? nullptr : j.col[4],
                                        j.sym ? nullptr : j.col[5], j.sym ? 1 : 0, j.cen_intervals.data(), j.cen_contained.data(), &j.n_contained, &bad_index, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    stage(j, "census");
}

// --overlap-ends: the kind of every record and the ends of every read it supports (raft_hip_overlap_ends_host), on the first context
// over the whole job's stream -- a multi-device or pre-split job is classified whole, before the split -- under the job's final
// symmetric flag, before prepare_input() writes window records over the query column.
void overlap_ends(Job &j)
{
    if (j.p.overlap_ends < 0) return;
    j.end_counts.resize((size_t)j.n_reads * 5); j.end_status.resize((size_t)j.n_reads);
    int64_t bad_index = -1;
    const int rc = raft_hip_overlap_ends_host(j.ctxs[0], j.n_reads, j.rl, j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.col[4], j.col[5], j.strand,
                                              j.p.overlap_ends, j.p.ends_min_ratio, j.sym ? 1 : 0, j.end_counts.data(), j.end_status.data(), nullptr,
                                              &j.end_sum, &bad_index, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    stage(j, "overlap_ends");
}

// --best-overlaps: the best overlap of every read end and whether it is mutual (raft_hip_best_overlaps_host), directly behind
// overlap_ends(): on the first context over the same whole stream under the same H, F and symmetric flag, with the reads that phase
// found contained left out (their status byte is the mask).
void best_overlaps(Job &j)
{
    if (!j.p.best_overlaps) return;
    j.best_partner.resize((size_t)j.n_reads * 2); j.best_span.resize((size_t)j.n_reads * 2); j.best_flags.resize((size_t)j.n_reads);
    std::vector<uint8_t> skip(j.end_status.size());
    for (size_t r = 0; r < skip.size(); ++r) skip[r] = j.end_status[r] == RAFT_HIP_END_READ_CONTAINED ? 1 : 0;
    int64_t bad_index = -1;
    const int rc = raft_hip_best_overlaps_host(j.ctxs[0], j.n_reads, j.rl, j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.col[4], j.col[5], j.strand,
                                               skip.data(), j.p.overlap_ends, j.p.ends_min_ratio, j.sym ? 1 : 0, j.best_partner.data(), j.best_span.data(),
                                               j.best_flags.data(), &j.best_sum, &bad_index, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    stage(j, "best_overlaps");
}

// --unitigs: the chains and cycles of the mutual best overlaps (raft_hip_unitigs_host), directly behind best_overlaps() on the
// arrays that phase holds.
void unitigs(Job &j)
{
    if (!j.p.unitigs) return;
    const size_t n = (size_t)j.n_reads;
    j.utg_unitig.resize(n); j.utg_index.resize(n); j.utg_order.resize(n); j.utg_reads.resize(n);
    j.utg_offset.resize(n); j.utg_off.resize(n + 1); j.utg_length.resize(n);
    j.utg_orient.resize(n); j.utg_circular.resize(n);
    int64_t bad_index = -1;
    const int rc = raft_hip_unitigs_host(j.ctxs[0], j.n_reads, j.rl, j.best_partner.data(), j.best_span.data(), j.best_flags.data(),
                                         j.utg_unitig.data(), j.utg_index.data(), j.utg_offset.data(), j.utg_orient.data(), j.utg_order.data(),
                                         j.utg_off.data(), j.utg_reads.data(), j.utg_length.data(), j.utg_circular.data(), &j.utg_sum, &bad_index,
                                         nullptr, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    stage(j, "unitigs");
}

// hifiasm writes its PAF grouped by query (reference README.md:36-38): a symmetric stream of at most four runs sorted by
// read id is handed over in its grouped form -- per run, where every read's records begin -- and the query column stays
// on the host (a third of the upload); any other stream goes up as it is.
// By default neither that nor the window records are prepared here: the engine's host pipeline derives both from the plain columns
// of a symmetric stream itself, chunk by chunk, beside the uploads of the chunks before (raft_hip.h "derived input"); made here
// they are a second and a third pass over the columns between the parse and the engine (19 ms for 4.4e7 records).
// RAFT_CLI_PREPARE=1 keeps them (A/B, and the grouped / window-record entry points through the CLI).
void prepare_input(Job &j)
{
    const bool prepare = j.sw.cli_prepare && j.ranks == 0;
    if (raft_cli::keeps_query_ids_with_lift(prepare, j.p.min_anchor, j.p.fragment_overlaps, j.p.fragment_paf)) j.ovl_qid.assign(j.col[0], j.col[0] + j.n_rec);   // (--repeat-overlaps, --fragment-overlaps and --fragment-paf read the query ids after the job)
    if (prepare && j.sym && j.n_rec > 0 && !j.sw.no_grouped) {
        j.rec_off.reset(new int64_t[(size_t)4 * ((size_t)j.n_reads + 1)]);
        if (raft_host_group_offsets(j.n_reads, j.n_rec, j.col[0], 4, &j.n_runs, j.rec_off.get()) != RAFT_HOST_OK) j.n_runs = 0;
        if (j.n_runs == 0 && j.devices.size() == 1 && j.n_rec < ((int64_t)1 << 29)) {
            // more than four runs (a PAF concatenated from more than two pairs of files): up to sixteen are still grouped input
            // for one device -- merged into one run on the device instead of falling to the counting sort
            j.rec_off.reset(new int64_t[(size_t)16 * ((size_t)j.n_reads + 1)]);
            if (raft_host_group_offsets(j.n_reads, j.n_rec, j.col[0], 16, &j.n_runs, j.rec_off.get()) != RAFT_HOST_OK) j.n_runs = 0;
        }
    }
    stage(j, "group_offsets");
    // ... and its records as window records: what profileCoverage uses of an interval is the windows it touches
    // (repeat.hpp:69-72), two 16-bit indices where reads stay below 65,535 windows -- one word per record goes up instead
    // of two.  They are written over the query column, which grouped input no longer needs.
    if (j.n_runs > 0 && j.p.reso <= 32767 && !j.sw.no_windows) {
        uint32_t *w = reinterpret_cast<uint32_t *>(const_cast<int32_t *>(j.col[0]));
        int64_t bad = -1;
        if (raft_host_pack_windows(j.n_rec, j.col[1], j.col[2], j.p.reso, w, &bad) == RAFT_HOST_OK) j.win = w;
        // (a negative coordinate or a window index beyond 16 bits: the coordinate columns go up, and the engine reports the former)
    }
    stage(j, "pack_windows");
}

// the inputs are page-locked in the form they go up in
void lock_inputs(Job &j)
{
    if (j.n_runs > 0) pin(j, j.rec_off.get(), (size_t)j.n_runs * ((size_t)j.n_reads + 1) * 8);
    if (j.win) pin(j, j.win, (size_t)j.n_rec * 4);
    else for (int k = j.n_runs > 0 ? 1 : 0; k < (j.sym ? 3 : 6); ++k) pin(j, j.col[k], (size_t)j.n_rec * 4);
    stage(j, "page-lock");
}

// The first attempt's coverage encoding (cli_plan.hpp first_cov_width; p.est_cov is the survey's by now): four-bit steps for
// grouped input and for plain columns that look like a handful of sorted runs, else one byte per window, or two from 40x on.
void choose_encoding(Job &j)
{
    const bool prepare = j.sw.cli_prepare && j.ranks == 0;
    const bool few_runs = j.sym && !prepare && j.n_rec > 0 && raft_cli::few_sorted_runs(j.col[0], j.n_rec);
    j.cov_width = raft_cli::first_cov_width(j.n_runs, few_runs, j.sw.no_delta4, j.ranks, j.p.est_cov);
}

// upload, pass and download of consecutive read ranges overlap, on every device named (one piece for small inputs)
int call_engine(Job &j, raft_hip_host_outputs *ho)
{
    raft_hip_ctx **ctxs = j.ctxs.data();
    const int32_t n_ctx = (int32_t)j.ctxs.size();
    if (j.ranks > 0)
        return raft_hip_run_presplit_local(ctxs, n_ctx, j.n_reads, j.rl, j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.col[4], j.col[5], ho, &j.s);
    if (j.win)
        return raft_hip_run_multi_windows(ctxs, n_ctx, j.n_reads, j.rl, j.n_rec, j.n_runs, j.rec_off.get(), j.win, j.sw.chunks, ho, &j.s);
    if (j.n_runs > 0)
        return raft_hip_run_multi_grouped(ctxs, n_ctx, j.n_reads, j.rl, j.n_rec, j.n_runs, j.rec_off.get(), j.col[1], j.col[2], j.sw.chunks, ho, &j.s);
    return raft_hip_run_multi(ctxs, n_ctx, j.n_reads, j.rl, j.n_rec, j.col[0], j.col[1], j.col[2], j.sym ? nullptr : j.col[3], j.sym ? nullptr : j.col[4],
                              j.sym ? nullptr : j.col[5], j.sw.chunks, ho, &j.s);
}

// The job, and the ladder behind it: an attempt that meets more windows at or above the limit than the exception list holds is
// followed by the one cli_plan.hpp next_attempt names, three at the most.
void run_engine(Job &j)
{
    const raft_cli::Capacities &c = j.cap;
    int rc = RAFT_HIP_OK;
    for (int64_t exc_cap = c.exc_cap0, attempt = 0; attempt < 3; ++attempt) {
        if ((int64_t)j.exc_i.size() != exc_cap) {          // (a retry with more room: the first size was made and page-locked beside the tokenising)
            if (!j.sw.no_pin) { (void)raft_hip_host_unregister(j.exc_i.data()); (void)raft_hip_host_unregister(j.exc_v.data()); }
            j.exc_i.resize((size_t)exc_cap); j.exc_v.resize((size_t)exc_cap);
            pin(j, j.exc_i.data(), j.exc_i.size() * 8); pin(j, j.exc_v.data(), j.exc_v.size() * 4);
        }
        if (raft_cli::cov_range_too_short(j.cov_width, c.n_win, j.cov8_locked)) {   // (a retry in a wider encoding than the array was page-locked for)
            if (!j.sw.no_pin) (void)raft_hip_host_unregister(j.cov8.get());
            j.cov8_locked = raft_cli::cov_bytes_needed(j.cov_width, c.n_win);
            pin(j, j.cov8.get(), (size_t)j.cov8_locked);
        }
        raft_hip_host_outputs ho{};
        ho.cov_offset = j.cov_off.data(); ho.cov8 = j.cov8.get(); ho.cov8_cap = c.n_win; ho.cov_width = j.cov_width;
        ho.cov_anchor = j.cov_anchor.data(); ho.anchor_cap = (int64_t)j.cov_anchor.size();
        ho.exc_index = j.exc_i.data(); ho.exc_value = j.exc_v.data(); ho.exc_cap = exc_cap;
        ho.rep_offset = j.rep_off.data(); ho.rep_s = j.rep_s.get(); ho.rep_e = j.rep_e.get(); ho.rep_cap = c.rep_cap;
        ho.frag_offset = j.frag_off.data(); ho.frag_begin = j.fb.get(); ho.frag_end = j.fe.get(); ho.frag_cap = c.frag_cap;
        rc = call_engine(j, &ho);
        j.n_exc = ho.n_exc;
        j.n_attempts = (int)attempt + 1;
        if (raft_cli::ladder_stops(rc, (int)attempt, j.n_exc, exc_cap)) break;
        const raft_cli::Attempt next = raft_cli::next_attempt(j.cov_width, exc_cap, j.n_exc, c.n_win);
        j.cov_width = next.cov_width;
        exc_cap = next.exc_cap;
    }
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, j.s.error_index));
    stage(j, "engine+fetch");
}

// --repeat-overlaps: the tokenised columns against the job's own repeat annotation -- the host arrays long_repeats.txt is written
// from, so it is the same call whichever way the job ran (one device or several, ranks, -e auto).  Both sides are classified; the
// reads' tallies follow the job's symmetric flag, as the census does.
void repeat_overlaps(Job &j)
{
    if (j.p.min_anchor <= 0) return;
    j.ovl_cls.resize((size_t)j.n_rec); j.ovl_flags.resize((size_t)j.n_reads);
    j.ovl_touch.resize((size_t)j.n_reads); j.ovl_repeat.resize((size_t)j.n_reads);
    if (!j.ovl_qid.empty()) j.col[0] = j.ovl_qid.data();
    int64_t bad_index = -1;
    const int rc = raft_hip_repeat_overlaps_host(j.ctxs[0], j.n_reads, j.rl, j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.col[4], j.col[5], j.sym ? 1 : 0,
                                                 j.p.min_anchor, j.rep_off[(size_t)j.n_reads], j.rep_off.data(), j.rep_s.get(), j.rep_e.get(),
                                                 j.ovl_cls.data(), j.ovl_touch.data(), j.ovl_repeat.data(), j.ovl_flags.data(), &j.ovl_sum, &bad_index, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    stage(j, "repeat_overlaps");
}

// --fragment-overlaps: the tokenised columns against the job's own fragment rows and repeat annotation -- the host arrays reads.fasta and
// long_repeats.txt are written from, so it is the same call whichever way the job ran (one device or several, ranks, -e auto): the
// whole-job arrays go to the first context.  Sides are counted under the job's symmetric flag, as the census counts them.
void fragment_overlaps(Job &j)
{
    if (!j.p.fragment_overlaps) return;
    const int64_t n_frag = j.frag_off[(size_t)j.n_reads];
    for (std::vector<int32_t> *v : {&j.frag_touch, &j.frag_span, &j.frag_contained, &j.frag_repeat}) v->resize((size_t)n_frag);
    if (!j.ovl_qid.empty()) j.col[0] = j.ovl_qid.data();
    const raft_hip_records rec{j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.col[4], j.col[5]};
    const raft_hip_frag_table table{n_frag, j.frag_off.data(), j.fb.get(), j.fe.get()};
    const raft_hip_frag_repeats repeats{j.rep_off[(size_t)j.n_reads], j.rep_off.data(), j.rep_s.get(), j.rep_e.get()};
    int64_t bad_index = -1;
    const int rc = raft_hip_frag_overlaps_host(j.ctxs[0], j.n_reads, j.rl, &rec, j.sym ? 1 : 0, &table, &repeats, j.frag_touch.data(), j.frag_span.data(),
                                               j.frag_contained.data(), j.frag_repeat.data(), nullptr, &j.frag_sum, &bad_index, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    stage(j, "fragment_overlaps");
}

// --fragment-paf: the job's kept stream lifted onto the job's own fragment rows -- the host arrays reads.fasta is written from, so it
// is the same call whichever way the job ran (one device or several, ranks, -e auto): the whole-job arrays go to the first context.
// A size query, the eight columns at that size, the call.
void fragment_paf(Job &j)
{
    if (!j.p.fragment_paf) return;
    if (!j.ovl_qid.empty()) j.col[0] = j.ovl_qid.data();
    const raft_hip_records rec{j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.col[4], j.col[5]};
    const raft_hip_frag_table table{j.frag_off[(size_t)j.n_reads], j.frag_off.data(), j.fb.get(), j.fe.get()};
    int64_t bad_index = -1;
    int rc = raft_hip_lift_overlaps_host(j.ctxs[0], j.n_reads, &rec, j.strand, &table, j.p.fragment_paf_min, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, &j.lift_sum, &bad_index, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    const size_t n_out = (size_t)j.lift_sum.n_out;
    if (n_out > 0) {
        for (auto &c : j.lift_col) c.resize(n_out);
        j.lift_rev.resize(n_out); j.lift_src.resize(n_out);
        rc = raft_hip_lift_overlaps_host(j.ctxs[0], j.n_reads, &rec, j.strand, &table, j.p.fragment_paf_min, (int64_t)n_out, j.lift_col[0].data(),
                                         j.lift_col[1].data(), j.lift_col[2].data(), j.lift_col[3].data(), j.lift_col[4].data(), j.lift_col[5].data(),
                                         j.lift_rev.data(), j.lift_src.data(), &j.lift_sum, &bad_index, nullptr);
        if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    }
    stage(j, "fragment_paf");
}

void write_fragment_paf(Job &j)
{
    if (raft_host_write_fragment_paf((j.p.prefix + ".fragments.paf").c_str(), j.reads, j.frag_off.data(), j.fb.get(), j.fe.get(), j.lift_sum.n_out,
                                     j.lift_col[0].data(), j.lift_col[1].data(), j.lift_col[2].data(), j.lift_col[3].data(), j.lift_col[4].data(),
                                     j.lift_col[5].data(), j.lift_rev.data(), j.lift_src.data(), j.lift_matches, j.lift_block) != RAFT_HOST_OK)
        die("ERROR, fragment_paf(), cannot write output files");
}

void write_fragment_overlaps(Job &j)
{
    std::vector<const char *> names((size_t)j.n_reads);
    for (int32_t i = 0; i < j.n_reads; ++i) names[(size_t)i] = raft_host_reads_name(j.reads, i);
    if (raft_host_write_fragments((j.p.prefix + ".fragments.tsv").c_str(), j.n_reads, names.data(), j.frag_off.data(), j.fb.get(), j.fe.get(),
                                  j.frag_touch.data(), j.frag_span.data(), j.frag_contained.data(), j.frag_repeat.data()) != RAFT_HOST_OK)
        die("ERROR, fragment_overlaps(), cannot write output files");
}

// --repeat-stats: the file is written from the job's own runs, beside long_repeats.txt; the rows come from the stats pass, which must
// have found the same number of runs
void write_repeat_stats(Job &j)
{
    const int64_t n_rep = j.rep_off[(size_t)j.n_reads];
    if (!j.rst_done || (int64_t)j.rst_flags.size() != n_rep)
        die("ERROR, repeat_stats(), the stats pass found " + std::to_string(j.rst_flags.size()) + " repeats, the job " + std::to_string(n_rep));
    std::vector<const char *> names((size_t)j.n_reads);
    for (int32_t i = 0; i < j.n_reads; ++i) names[(size_t)i] = raft_host_reads_name(j.reads, i);
    if (raft_host_write_repeat_stats((j.p.prefix + ".long_repeats.stats.tsv").c_str(), j.n_reads, names.data(), j.rep_off.data(), j.rep_s.get(), j.rep_e.get(),
                                     j.rst_flags.data(), j.rst_windows.data(), j.rst_cov_sum.data(), j.rst_min.data(), j.rst_max.data(), j.rst_high.data(),
                                     j.rst_touch.data(), j.rst_span.data(), j.rst_inside.data()) != RAFT_HOST_OK)
        die("ERROR, repeat_stats(), cannot write output files");
}

void write_repeat_overlaps(Job &j)
{
    const Params &p = j.p;
    std::vector<const char *> names((size_t)j.n_reads);
    for (int32_t i = 0; i < j.n_reads; ++i) names[(size_t)i] = raft_host_reads_name(j.reads, i);
    if (raft_host_write_repeat_overlaps((p.prefix + ".repeat_overlaps.tsv").c_str(), (p.prefix + ".repeat_overlaps.records.tsv").c_str(), j.n_reads,
                                        names.data(), j.rl, j.ovl_touch.data(), j.ovl_repeat.data(), j.ovl_flags.data(), j.n_rec, j.col[0], j.col[1],
                                        j.col[2], j.col[3], j.col[4], j.col[5], j.ovl_cls.data()) != RAFT_HOST_OK)
        die("ERROR, repeat_overlaps(), cannot write output files");
}

void report(Job &j)
{
    const raft_hip_summary &s = j.s;
    if (j.sw.timing) fprintf(stderr, "TIMING devices_used %d input %s attempts %d\n", s.n_devices_used, raft_cli::input_label(j.ranks, j.win != nullptr, j.n_runs, j.sym), j.n_attempts);
    if (j.sw.timing) fprintf(stderr, "TIMING coverage_encoding %s\n", raft_cli::encoding_label(j.cov_width));
    fprintf(stdout, "INFO, Symmetric overlaps %d \n", s.symmetric);            // chop.hpp:189-190
    fprintf(stdout, "INFO, length of alignments  %d()\n", (int)s.n_records);
    fprintf(stdout, "high_cov %d\n", s.high_cov);                              // repeat.hpp:91
}

void write_read_stats(Job &j)
{
    const Params &p = j.p;
    std::vector<const char *> names((size_t)j.n_reads);
    for (int32_t i = 0; i < j.n_reads; ++i) names[(size_t)i] = raft_host_reads_name(j.reads, i);
    if (raft_host_write_read_stats((p.prefix + ".read_stats.tsv").c_str(), j.n_reads, names.data(), j.rl, p.reso, j.cen_intervals.data(), j.cen_contained.data(),
                                   j.rs_sum.data(), j.rs_max.data(), j.rs_high.data(), j.rep_off.data(), j.frag_off.data()) != RAFT_HOST_OK)
        die("ERROR, read_stats(), cannot write output files");
}

void write_low_coverage(Job &j)
{
    const Params &p = j.p;
    std::vector<const char *> names((size_t)j.n_reads);
    for (int32_t i = 0; i < j.n_reads; ++i) names[(size_t)i] = raft_host_reads_name(j.reads, i);
    if (raft_host_write_low_coverage((p.prefix + ".low_coverage.bed").c_str(), j.n_reads, names.data(), j.low_off.data(), j.low_s.data(), j.low_e.data(),
                                     j.rl, p.reso) != RAFT_HOST_OK)
        die("ERROR, low_coverage(), cannot write output files");
}

// the four output files are independent: the FASTA is written beside the coverage/repeat tables
void write_outputs(Job &j)
{
    const Params &p = j.p;
    const raft_hip_summary &s = j.s;
    j.fasta_writer = std::thread([&j] { j.fasta_rc = raft_host_write_fasta(j.fasta_out.c_str(), j.reads, j.frag_off.data(), j.fb.get(), j.fe.get()); });
    const int cov_rc = j.cov_width == RAFT_HIP_COV_DELTA4
        ? raft_host_write_coverage_d4((p.prefix + ".coverage.txt").c_str(), j.n_reads, p.reso, j.cov_off.data(), j.cov8.get(), j.cov_anchor.data(), j.n_exc,
                                      j.exc_i.data(), j.exc_v.data())
        : raft_host_write_coverage_packed_w(j.cov_width, (p.prefix + ".coverage.txt").c_str(), j.n_reads, p.reso, j.cov_off.data(), j.cov8.get(), j.n_exc,
                                            j.exc_i.data(), j.exc_v.data());
    if (cov_rc != RAFT_HOST_OK ||
        raft_host_write_repeats((p.prefix + ".long_repeats.txt").c_str(), (p.prefix + ".long_repeats.bed").c_str(), j.reads,
                                j.rep_off.data(), j.rep_s.get(), j.rep_e.get()) != RAFT_HOST_OK) {
        die("ERROR, repeat_annotate(), cannot write output files");
    }
    if (p.read_stats) write_read_stats(j);
    if (p.low_cov >= 0) write_low_coverage(j);
    if (p.min_anchor > 0) write_repeat_overlaps(j);
    if (p.fragment_overlaps) write_fragment_overlaps(j);
    if (p.repeat_stats) write_repeat_stats(j);
    if (p.overlap_ends >= 0 &&
        raft_host_write_overlap_ends((p.prefix + ".overlap_ends.tsv").c_str(), j.reads, j.end_counts.data(), j.end_status.data()) != RAFT_HOST_OK)
        die("ERROR, overlap_ends(), cannot write output files");
    if (p.best_overlaps &&
        raft_host_write_best_overlaps((p.prefix + ".best_overlaps.tsv").c_str(), j.reads, j.best_partner.data(), j.best_span.data(), j.best_flags.data()) != RAFT_HOST_OK)
        die("ERROR, best_overlaps(), cannot write output files");
    if (p.unitigs &&
        raft_host_write_unitigs(p.prefix.c_str(), j.reads, j.utg_sum.unitigs, j.utg_unitig.data(), j.utg_index.data(), j.utg_offset.data(),
                                j.utg_orient.data(), j.utg_order.data(), j.utg_off.data(), j.utg_reads.data(), j.utg_length.data(),
                                j.utg_circular.data()) != RAFT_HOST_OK)
        die("ERROR, unitigs(), cannot write output files");
    if (p.fragment_paf) write_fragment_paf(j);
    stage(j, "write_tables");
    // repeat.hpp:173-178 (total_windows is an int in the reference; identical below 2^31 windows)
    const double cpw = (double)s.total_coverage / (double)s.total_windows;
    fprintf(stdout, "coverage per window is %f \n", cpw);
    fprintf(stdout, "coverage per window/average coverage is %f \n", cpw / p.est_cov);
    fprintf(stdout, "fraction_of_repeat_length %f \n", (double)s.total_repeat_length / (double)s.total_read_length);

    j.fasta_writer.join();
    if (j.fasta_rc != RAFT_HOST_OK) die("ERROR, break_reads(), cannot write " + j.fasta_out);
    stage(j, "write_fasta");
    fflush(stdout);
}

void print_totals(Job &j, int argc, char *argv[])
{
    const std::chrono::duration<double> wct = std::chrono::system_clock::now() - j.t_start;
    std::cout << "INFO, main(), program completed after " << wct.count() << " seconds\n";
    std::cout.flush();
    fprintf(stdout, "INFO, %s(), CMD:", "main");   // main.cpp:81-84
    for (int i = 0; i < argc; ++i) fprintf(stdout, " %s", argv[i]);
    fflush(stdout);
    std::cout << "\n";
    if (j.filtered)
        std::cout << raft_cli::filter_overlaps_line(j.p.min_identity, j.p.min_overlap, j.flt_sum.n_records, j.flt_sum.n_kept, j.flt_sum.below_identity,
                                                    j.flt_sum.below_span) << "\n";
    if (j.p.read_stats) std::cout << "INFO, read_stats(), contained reads = " << j.n_contained << " of " << j.n_reads << "\n";
    if (j.p.low_cov >= 0)
        std::cout << "INFO, low_coverage(), low_cov = " << j.p.low_cov << ", runs = " << j.low_sum.n_runs << ", reads with an interior run = "
                  << j.low_sum.reads_interior << ", uncovered reads = " << j.low_sum.reads_uncovered << " of " << j.n_reads << "\n";
    if (j.p.min_anchor > 0)
        std::cout << "INFO, repeat_overlaps(), min_anchor = " << j.p.min_anchor << ", records = " << j.ovl_sum.n_records << ", query side in a repeat = "
                  << j.ovl_sum.q_repeat << ", target side = " << j.ovl_sum.t_repeat << ", both = " << j.ovl_sum.both_repeat << ", contained reads = "
                  << j.ovl_sum.reads_contained << ", contained only inside repeats = " << j.ovl_sum.reads_repeat_contained << "\n";
    if (j.p.fragment_overlaps)
        std::cout << raft_cli::fragment_overlaps_line(j.frag_sum.n_fragments, j.frag_sum.frags_spanned, j.frag_sum.frags_contained,
                                                      j.frag_sum.frags_contained_repeat, j.frag_sum.reads_whole_spanned, j.frag_sum.reads_all_contained,
                                                      j.n_reads) << "\n";
    if (j.p.repeat_stats)
        std::cout << raft_cli::repeat_stats_line(j.rst_sum.n_runs, j.rst_sum.runs_interior, j.rst_sum.runs_spanned, j.rst_sum.interior_spanned,
                                                 j.rst_sum.runs_touched, j.rst_sum.sides_inside) << "\n";
    if (j.p.overlap_ends >= 0)
        std::cout << raft_cli::overlap_ends_line(j.p.overlap_ends, j.p.ends_min_ratio, j.end_sum.n_records, j.end_sum.kind_internal,
                                                 j.end_sum.kind_query_contained, j.end_sum.kind_target_contained, j.end_sum.kind_end3 + j.end_sum.kind_end5,
                                                 j.end_sum.kind_self, j.end_sum.kind_invalid, j.end_sum.reads_contained,
                                                 j.end_sum.reads_dead5 + j.end_sum.reads_dead3, j.end_sum.reads_isolated, j.n_reads) << "\n";
    if (j.p.best_overlaps)
        std::cout << raft_cli::best_overlaps_line(j.best_sum.n_records, j.best_sum.candidates, j.best_sum.left_out, j.best_sum.ends_best,
                                                  j.best_sum.ends_mutual, j.best_sum.reads_both_mutual, j.best_sum.reads_no_best,
                                                  j.best_sum.reads_skipped, j.n_reads) << "\n";
    if (j.p.unitigs)
        std::cout << raft_cli::unitigs_line(j.utg_sum.reads_in, j.utg_sum.reads_skipped, j.utg_sum.unitigs, j.utg_sum.singletons, j.utg_sum.circular,
                                            j.utg_sum.longest_reads, j.utg_sum.longest_length, j.utg_sum.total_length,
                                            raft_cli::unitig_n50(j.utg_length.data(), j.utg_sum.unitigs)) << "\n";
    if (j.p.fragment_paf)
        std::cout << raft_cli::fragment_paf_line(j.p.fragment_paf_min, j.lift_sum.n_records, j.lift_sum.n_out, j.lift_sum.records_cut,
                                                 j.lift_sum.records_none, j.lift_sum.pairs_dropped, j.lift_sum.most_per_record) << "\n";
    stage(j, "stdout");
    if (j.sw.timing) {
        timespec ts{};
        clock_gettime(CLOCK_REALTIME, &ts);
        fprintf(stderr, "TIMING %-16s %8.3f s\n", "main() total", std::chrono::duration<double>(std::chrono::steady_clock::now() - j.t_main).count());
        fprintf(stderr, "TIMING %-16s %lld.%03ld\n", "leaving-at", (long long)ts.tv_sec, ts.tv_nsec / 1000000);
    }
}

} // namespace

int main(int argc, char *argv[])
{
    Job job;
    g_job = &job;
    parse_options(job, argc, argv);
    print_params(job);
    check_inputs(job);
    fill_engine_params(job);
    read_switches(job);
    start_clock(job);
    start_devices(job);
    start_paf_read(job);
    load_reads(job);
    start_output_prep(job);
    parse_paf(job);
    await_devices(job);
    filter_overlaps(job);
    hand_over_symmetric_flag(job);
    survey(job);
    census(job);
    overlap_ends(job);
    best_overlaps(job);
    unitigs(job);
    prepare_input(job);
    lock_inputs(job);
    choose_encoding(job);
    run_engine(job);
    repeat_overlaps(job);
    fragment_overlaps(job);
    fragment_paf(job);
    report(job);
    write_outputs(job);
    print_totals(job, argc, argv);
    raft_host_text *const paf_text = job.paf_text;
    raft_host_paf *const paf = job.paf;
    raft_host_reads *const reads = job.reads;
    const std::vector<raft_hip_ctx *> &ctxs = job.ctxs;
    // Everything is written and closed.  Unmapping a GB of reads, freeing the device buffers and tearing the HIP runtime
    // down cost 0.2-0.3 s of a run that takes a second: leave that to the kernel's process exit.
    const bool out_ok = fflush(stdout) == 0 && !ferror(stdout) && std::cout.good();
    fflush(stderr);
    if (!out_ok) _exit(1);                           // a failed stdout write (closed pipe, full disk) is not a success
    // The fast exit skips atexit handlers and static destructors, which tools that finalise at exit rely on (rocprofv3 /
    // rocprofiler-sdk traces, gcov / llvm-cov counters, sanitizer reports): it is off whenever such a tool shows in
    // the environment, and RAFT_CLEAN_EXIT=1 turns it off by hand.
    auto has = [](const char *v) { const char *e = getenv(v); return e && *e; };
    const char *preload = getenv("LD_PRELOAD");
    const bool tooling = has("RAFT_CLEAN_EXIT") || has("ROCP_TOOL_LIBRARIES") || has("ROCPROFILER_REGISTER_FORCE_LOAD") ||
                         has("HSA_TOOLS_LIB") || has("ROCP_TOOL_LIB") || has("LLVM_PROFILE_FILE") || has("GCOV_PREFIX") ||
                         has("ASAN_OPTIONS") || has("LSAN_OPTIONS") || has("UBSAN_OPTIONS") ||
                         (preload && (strstr(preload, "rocprof") || strstr(preload, "asan") || strstr(preload, "tsan")));
    if (!tooling) _exit(0);
    if (paf_text) raft_host_text_free(paf_text);     // (the clean exit gives everything back: leak checkers see none)
    raft_host_paf_free(paf);
    raft_host_reads_free(reads);
    for (raft_hip_ctx *c : ctxs) raft_hip_destroy(c);
    return 0;
}
