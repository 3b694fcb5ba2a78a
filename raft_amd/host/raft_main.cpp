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
#include "../../include/raft_hip_cc.h"
#include "../../include/raft_host_cc.h"
#include "../../include/raft_hip_sg.h"
#include "../../include/raft_host_sg.h"
#include "../../include/raft_hip_ctn.h"
#include "../../include/raft_host_ctn.h"
#include "../../include/raft_hip_cln.h"
#include "../../include/raft_host_cln.h"
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

using raft_cli::Options;            // the command line as parsed (cli_plan.hpp)

struct Switches {                  // the environment, as read_switches() found it
    bool timing = false, no_warm_up = false, no_pin = false, no_delta4 = false, cli_prepare = false, no_grouped = false, no_windows = false;
    int context_width = 4;         // the width the first context has outside the survey
    int chunks = 0;                // 0: the engine decides (one piece for small inputs)
};

// What each optional output owns: one struct per row of kExtras (below), one member of the Job each.
// --min-identity / --min-overlap: what the filter counted, and the side columns of the kept records (strand; PAF fields 10 and 11)
struct FilterOut { raft_hip_flt_summary sum{}; std::vector<uint8_t> strand; std::vector<int32_t> matches, block; };
// --read-stats: the survey's coverage summary and the census of the record stream
struct ReadStatsOut { std::vector<int64_t> sum; std::vector<int32_t> max, high, intervals; std::vector<uint8_t> contained; int64_t n_contained = 0; };
struct LowCovOut { std::vector<int64_t> off; std::vector<int32_t> s, e; raft_hip_low_summary sum{}; };   // --low-cov: the survey's low-coverage runs
struct RepeatOverlapsOut { std::vector<uint8_t> cls, flags; std::vector<int32_t> touch, repeat; raft_hip_ovl_summary sum{}; };   // --repeat-overlaps: per record, per read
struct FragmentOverlapsOut { std::vector<int32_t> touch, span, contained, repeat; raft_hip_frag_summary sum{}; };   // --fragment-overlaps: per fragment
// --repeat-stats: per repeat run of the stats pass the sides that touch, span and lie inside it, its coverage, its flags
struct RepeatStatsOut { std::vector<int32_t> touch, span, inside, windows, min, max, high; std::vector<int64_t> cov_sum; std::vector<uint8_t> flags; raft_hip_rst_summary sum{}; bool done = false; };
struct EndsOut { std::vector<int32_t> counts; std::vector<uint8_t> status; raft_hip_end_summary sum{}; };   // --overlap-ends: the reads' counts and status
struct BestOut { std::vector<int32_t> partner, span; std::vector<uint8_t> flags; raft_hip_best_summary sum{}; };   // --best-overlaps: per read end, per read
// --unitigs: per read the unitig, the place in it, the offset and the orientation; the layout order; per unitig size, length, circular
struct UnitigOut { std::vector<int32_t> unitig, index, order, reads; std::vector<int64_t> offset, off, length; std::vector<uint8_t> orient, circular; raft_hip_utg_summary sum{}; };
// --components: per read the component and the degree; per component the smallest read, the reads, the bases, the sides
struct ComponentsOut { std::vector<int32_t> component, degree, first, reads; std::vector<int64_t> bases, sides; raft_hip_cc_summary sum{}; };
// --string-graph: per read end the arcs and the survivors, per read the flag byte; the surviving edges (nodes and span)
struct StringGraphOut { std::vector<int32_t> arcs, kept, u, w, span; std::vector<uint8_t> flags; raft_hip_sg_summary sum{}; };
// --containment: per read the parent with the place in it, the root with the place in it, the depth, the children, the flag byte; per root its tree
struct ContainmentOut { std::vector<int32_t> parent, pos, span, root, root_pos, depth, children, tree_reads; std::vector<int64_t> tree_bases; std::vector<uint8_t> flags; raft_hip_ctn_summary sum{}; };
// ... with --unitigs: per read the unitig, the start and the orientation; per unitig the reads, the bases and the depth
struct PlaceOut { std::vector<int32_t> unitig, reads; std::vector<int64_t> start, bases, permille; std::vector<uint8_t> orient; raft_hip_place_summary sum{}; };
// --graph-clean: per edge of string_graph()'s list the state, per read the state and the round, per read end the degrees before, the arcs the
// weak cut took and the degrees after, the cleaned table; the live edges; the unitigs of the cleaned table
struct GraphCleanOut { std::vector<uint8_t> edge_state, read_state, read_round, flags; std::vector<int32_t> arcs, weak, kept, partner, span, u, w, edge_span; raft_hip_cln_summary sum{}; UnitigOut utg; };
struct LiftOut { std::vector<int32_t> col[6], src; std::vector<uint8_t> rev; raft_hip_lift_summary sum{}; };   // --fragment-paf: the eight columns of the lifted stream

struct Job {
    Options p;
    raft_cli::Request rq{};        // what the options ask for between them (read_switches)
    const char *reads_fn = nullptr, *paf_fn = nullptr;
    std::string fasta_out;
    raft_hip_params hp{};
    Switches sw;
    bool prepare = false;          // group offsets and window records are made here (RAFT_CLI_PREPARE on a job without ranks)
    std::chrono::system_clock::time_point t_start;              // the reference's timer
    std::chrono::steady_clock::time_point t_main, t_prev;       // the stage clock
    // the devices: context d is on devices[d]; ranks > 0: the pre-split job
    std::vector<int> devices;
    int ranks = 0;
    std::vector<raft_hip_ctx *> ctxs;
    std::vector<int> create_rc;
    std::promise<void> devices_up_p;
    std::shared_future<void> devices_up;
    // the inputs; behind the filter n_rec, col, the symmetric flag and the side columns are the kept stream's
    raft_host_text *paf_text = nullptr;
    int paf_text_rc = RAFT_HOST_OK;
    raft_host_reads *reads = nullptr;
    int32_t n_reads = 0;
    const int32_t *rl = nullptr;
    std::vector<const char *> names;                            // the reads' names, for the writers that take them (names())
    raft_host_paf *paf = nullptr;
    int64_t n_rec = 0;
    const int32_t *col[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};    // qid, qs, qe, tid, ts, te
    const uint8_t *strand = nullptr;                            // the strand byte of every record, where Request::strand asked for it
    const int32_t *matches = nullptr, *block = nullptr;         // PAF fields 10 and 11 of the kept records (Request::quality_kept)
    std::vector<int32_t> qid_kept;                              // the query column as tokenised, where prepare_input writes over it (Request::keep_query_ids)
    // the optional outputs, in the order of kExtras
    FilterOut flt; ReadStatsOut rs; LowCovOut low; RepeatOverlapsOut ovl; FragmentOverlapsOut frag;
    RepeatStatsOut rst; EndsOut ends; BestOut best; UnitigOut utg; ComponentsOut cc; StringGraphOut sg; ContainmentOut ctn; PlaceOut plc; LiftOut lift; GraphCleanOut cln;
    // the arrays everything comes back in (made and page-locked on out_prep)
    raft_cli::Capacities cap;
    std::vector<int64_t> cov_off, rep_off, frag_off;
    std::unique_ptr<uint8_t[]> cov8;
    int64_t cov8_locked = 0;                  // the bytes of cov8 that are page-locked (cli_plan.hpp cov_bytes_needed)
    std::unique_ptr<int32_t[]> rep_s, rep_e, fb, fe;
    std::vector<int64_t> exc_i;
    std::vector<int32_t> exc_v;
    std::vector<int32_t> cov_anchor;          // the four-bit step encoding's block anchors (cov_width = RAFT_HIP_COV_DELTA4)
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

[[noreturn]] void print_help(const Options &p) // main.cpp:7-19
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

// How a phase on the device ends: an error is the engine's, in its words; else the stage clock moves on.
void done(Job &j, int rc, int64_t bad_index, const char *label)
{
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    stage(j, label);
}

// The stream's columns as a call takes them: all six; without the target's coordinates for a call that counts sides under the
// symmetric flag; without the target columns for a pass over a symmetric stream.
enum class Targets { all, ids, none };

raft_hip_records records(const Job &j, Targets t = Targets::all)
{
    return {j.n_rec, j.col[0], j.col[1], j.col[2], t == Targets::none ? nullptr : j.col[3], t == Targets::all ? j.col[4] : nullptr, t == Targets::all ? j.col[5] : nullptr};
}

// the reads' names for the writers that take them as an array: made at the first call
const char *const *names(Job &j)
{
    for (int32_t i = (int32_t)j.names.size(); i < j.n_reads; ++i) j.names.push_back(raft_host_reads_name(j.reads, i));
    return j.names.data();
}

void parse_options(Job &j, int argc, char *argv[])
{
    Options &p = j.p;
    // (the short options and their quirks are the reference's; the long options are this program's own, the rows of cli_plan.hpp's
    // list of tables, counted through by every_long_option(k), and behind them the rows of its open table: getopt_long returns 0 for
    // them and says which row)
    constexpr size_t n_every = raft_cli::every_long_option_count(), n_long = n_every + raft_cli::kOpenLongOptionCount;
    struct option long_options[n_long + 1] = {};
    for (size_t k = 0; k < n_every; ++k) long_options[k] = {raft_cli::every_long_option(k).name, raft_cli::every_long_option(k).parse ? required_argument : no_argument, nullptr, 0};
    for (size_t k = n_every; k < n_long; ++k) long_options[k] = {raft_cli::kOpenLongOptions[k - n_every].name, raft_cli::kOpenLongOptions[k - n_every].parse ? required_argument : no_argument, nullptr, 0};
    int option, row = 0;
    while ((option = getopt_long(argc, argv, "r:e:m:l:i:p:f:v:o:", long_options, &row)) != -1) {
        switch (option) {
        case 0: if (!raft_cli::set_long_option((size_t)row < n_every ? raft_cli::every_long_option((size_t)row) : raft_cli::kOpenLongOptions[(size_t)row - n_every], optarg, &p)) print_help(p); break;
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
    if (!raft_cli::usage_ok(p)) print_help(p);
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
    const Options &p = j.p;
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
    const Options &p = j.p;
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
    // ... and what the options ask for between them, under these switches: decided here, read everywhere else
    j.prepare = sw.cli_prepare && j.ranks == 0;
    j.rq = raft_cli::request(j.p, j.prepare);
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
    const Options &p = j.p;
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
    if (rc == RAFT_HOST_OK) rc = raft_host_paf_parse_with(j.paf_text, j.reads, j.rq.paf_columns, &j.paf, bad, sizeof bad);
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

// Side columns that must follow the kept records ride through the filter in its id slots: the filter copies its id columns without
// using them as indices (include/raft_hip_flt.h), so one more call of its host form under the same P and L compacts `q` in the
// query-id slot and, where there is one, `t` in the target-id slot; what it writes for the other columns is dropped.
void keep_side_columns(Job &j, std::vector<int32_t> &q, std::vector<int32_t> *t)
{
    std::vector<int32_t> drop[5];
    for (int k = 0; k < (t ? 4 : 5); ++k) drop[k].resize((size_t)j.n_rec);
    raft_hip_flt_summary sum{};
    const int rc = raft_hip_filter_overlaps_host(j.ctxs[0], j.n_rec, q.data(), j.col[1], j.col[2], t ? t->data() : j.col[3], j.col[4], j.col[5],
                                                 raft_host_paf_quality(j.paf, 0), raft_host_paf_quality(j.paf, 1), j.p.min_identity, j.p.min_overlap,
                                                 q.data(), drop[0].data(), drop[1].data(), t ? t->data() : drop[4].data(), drop[2].data(), drop[3].data(),
                                                 &sum, nullptr);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, -1));
    q.resize((size_t)sum.n_kept);
    if (t) t->resize((size_t)sum.n_kept);
}

// --min-identity / --min-overlap: the records that pass (include/raft_hip_flt.h) are compacted in place, on the first context, before
// anything else sees the stream -- the survey, the census, the split of a multi-device or pre-split job, every query: the job is the
// job on a file of the kept lines.  Without the options nothing happens here.  The strand (--overlap-ends, --fragment-paf) and PAF
// fields 10 and 11 (--fragment-paf, for the writer) follow the kept records.
void filter_overlaps(Job &j)
{
    if (!j.rq.filter) return;
    j.out_prep.join();                                  // (its raft_hip_reserve uses the context this call runs on)
    FilterOut &f = j.flt;
    if (j.rq.strand) {                                  // (first: the side columns go through beside the columns as tokenised)
        std::vector<int32_t> wide(j.strand, j.strand + j.n_rec);           // the strand bytes widened to int32
        keep_side_columns(j, wide, nullptr);
        f.strand.assign(wide.begin(), wide.end());
        j.strand = f.strand.data();
    }
    if (j.rq.quality_kept) {
        const int32_t *m = raft_host_paf_quality(j.paf, 0), *b = raft_host_paf_quality(j.paf, 1);
        f.matches.assign(m, m + j.n_rec); f.block.assign(b, b + j.n_rec);
        keep_side_columns(j, f.matches, &f.block);
        j.matches = f.matches.data(); j.block = f.block.data();
    }
    int32_t *out[6];
    for (int k = 0; k < 6; ++k) out[k] = const_cast<int32_t *>(j.col[k]);
    const int rc = raft_hip_filter_overlaps_host(j.ctxs[0], j.n_rec, j.col[0], j.col[1], j.col[2], j.col[3], j.col[4], j.col[5],
                                                 raft_host_paf_quality(j.paf, 0), raft_host_paf_quality(j.paf, 1), j.p.min_identity, j.p.min_overlap,
                                                 out[0], out[1], out[2], out[3], out[4], out[5], &f.sum, nullptr);
    if (rc == RAFT_HIP_OK) j.n_rec = f.sum.n_kept;
    done(j, rc, -1, "filter_overlaps");
}

// the symmetric flag of the stream the job runs on: the tokeniser's, or the filter's for the kept stream
bool stream_symmetric(const Job &j) { return j.rq.filter ? j.flt.sum.symmetric != 0 : raft_host_paf_symmetric(j.paf) != 0; }

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
    ReadStatsOut &o = j.rs;
    o.sum.resize((size_t)j.n_reads); o.max.resize((size_t)j.n_reads); o.high.resize((size_t)j.n_reads);
    const int32_t high_cov = (int32_t)(est_cov * j.p.cov_mul);          // (the job's: repeat.hpp:89-90)
    const int rc = raft_hip_read_stats(j.ctxs[0], std::max(high_cov, 1), o.sum.data(), o.max.data(), o.high.data(), nullptr);
    if (high_cov < 1)                                                    // (every window is at or above a threshold below 1)
        for (int32_t i = 0; i < j.n_reads; ++i) o.high[(size_t)i] = (int32_t)(((int64_t)j.rl[i] + j.p.reso - 1) / j.p.reso);
    return rc;
}

// --low-cov: the low-coverage runs of the pass that has just run.  The run arrays start at cli_plan.hpp's first size; a set with more
// runs says so (RAFT_HIP_ERR_TOO_LARGE and the number) and is asked once more.
int survey_low_coverage(Job &j, int64_t n_win)
{
    LowCovOut &o = j.low;
    o.off.resize((size_t)j.n_reads + 1);
    int64_t cap = raft_cli::low_run_capacity0(n_win, j.n_reads);
    int rc = RAFT_HIP_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        o.s.resize((size_t)cap); o.e.resize((size_t)cap);
        rc = raft_hip_low_coverage(j.ctxs[0], j.p.low_cov, raft_cli::kLowUncoveredPermille, cap, o.off.data(), o.s.data(), o.e.data(), nullptr, nullptr,
                                   &o.sum, nullptr);
        if (rc != RAFT_HIP_ERR_TOO_LARGE) break;
        cap = o.sum.n_runs;
    }
    return rc;
}

// --repeat-stats: one row per repeat run of the pass that has just run -- its own annotation, its coverage, the tokenised columns
// under the job's symmetric flag as census() hands them over --, before prepare_input() writes window records over the query column.
int survey_repeat_stats(Job &j, int est_cov, int64_t n_repeats, int64_t *bad_index)
{
    RepeatStatsOut &o = j.rst;
    for (std::vector<int32_t> *v : {&o.touch, &o.span, &o.inside, &o.windows, &o.min, &o.max, &o.high}) v->resize((size_t)n_repeats);
    o.cov_sum.resize((size_t)n_repeats); o.flags.resize((size_t)n_repeats);
    const raft_hip_records rec = records(j, j.sym ? Targets::ids : Targets::all);
    o.done = true;
    return raft_hip_repeat_stats_host(j.ctxs[0], j.n_reads, j.rl, &rec, j.sym ? 1 : 0, -1, nullptr, nullptr, nullptr,
                                      raft_cli::repeat_stats_threshold(est_cov, j.p.cov_mul), o.touch.data(), o.span.data(), o.inside.data(),
                                      o.windows.data(), o.min.data(), o.max.data(), o.high.data(), o.cov_sum.data(), o.flags.data(), &o.sum, bad_index,
                                      nullptr);
}

// one one-piece pass of the survey on the first context (rc: of the settings it runs under), the columns as its symmetric flag has them
void survey_pass(Job &j, int rc, raft_hip_summary *ss)
{
    const raft_hip_records r = records(j, j.hp.symmetric_mode != 1 ? Targets::all : Targets::none);
    if (rc == RAFT_HIP_OK) rc = raft_hip_run_host(j.ctxs[0], j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te);
    if (rc == RAFT_HIP_OK) rc = raft_hip_finish(j.ctxs[0], ss);
    if (rc != RAFT_HIP_OK) die(engine_error(j, rc, ss->error_index));
}

// -e auto: the survey.  cov[] does not depend on est_cov, so one one-piece pass on the first context under the placeholder holds
// the number -e stands for: its coverage histogram is made on the device (32 KiB come back instead of cov[]) and the estimate
// read from it (raft_hip.h).  The pass writes two-byte codes and no cut points -- nothing of it is fetched --, and its
// overlap_length is 0: which fragments there are depends on the repeats, hence on the placeholder, and RAFT_HIP_ERR_FRAGMENT of
// the survey would not be the job's.  Every other data error (ids, coordinates, lengths) is the one the job would report, in
// its words.  With several devices or ranks the survey still runs in one piece on the first: one more upload of the columns.
// --read-stats: the per-read table.  Its coverage summary (raft_hip_read_stats) is taken from the same survey pass, right behind
// the histogram; without -e auto one such pass -- the survey's recipe -- runs here for it.  The job itself runs as it does
// without the option.  --low-cov: the same, for the low-coverage runs (raft_hip_low_coverage), behind the two.
// --repeat-stats: the table of the repeat runs (raft_hip_repeat_stats_host) needs coverage AND annotation under the job's final est_cov:
// with -e auto one more pass of the same recipe runs under the estimate (one more upload of the columns), the table right behind it.
void survey(Job &j)
{
    Options &p = j.p;
    if (!j.rq.survey) return;
    raft_hip_ctx *ctx = j.ctxs[0];
    SurveySettings settings{ctx, j.sw.context_width};
    raft_hip_params sp = j.hp;
    sp.overlap_length = 0;
    raft_hip_summary ss{};
    ss.error_index = -1;
    survey_pass(j, settings.apply(sp), &ss);
    int rc = RAFT_HIP_OK;
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
        if (j.rq.repeat_stats_second_pass) {
            sp.est_cov = est.est_cov;
            survey_pass(j, raft_hip_set_params(ctx, &sp), &ss);
        }
        int64_t bad_index = -1;
        rc = survey_repeat_stats(j, est.est_cov, ss.n_repeats, &bad_index);
        if (rc != RAFT_HIP_OK) die(engine_error(j, rc, bad_index));
    }
    if (rc == RAFT_HIP_OK) rc = settings.restore_outputs();
    done(j, rc, -1, "estimate");
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
    ReadStatsOut &o = j.rs;
    o.intervals.resize((size_t)j.n_reads); o.contained.resize((size_t)j.n_reads);
    const raft_hip_records r = records(j, j.sym ? Targets::ids : Targets::all);
    int64_t bad_index = -1;
    const int rc = raft_hip_census_host(j.ctxs[0], j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, j.sym ? 1 : 0,
                                        o.intervals.data(), o.contained.data(), &o.n_contained, &bad_index, nullptr);
    done(j, rc, bad_index, "census");
}

// --overlap-ends: the kind of every record and the ends of every read it supports (raft_hip_overlap_ends_host), on the first context
// over the whole job's stream -- a multi-device or pre-split job is classified whole, before the split -- under the job's final
// symmetric flag, before prepare_input() writes window records over the query column.
void overlap_ends(Job &j)
{
    EndsOut &o = j.ends;
    o.counts.resize((size_t)j.n_reads * 5); o.status.resize((size_t)j.n_reads);
    const raft_hip_records r = records(j);
    int64_t bad_index = -1;
    const int rc = raft_hip_overlap_ends_host(j.ctxs[0], j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, j.strand,
                                              j.p.overlap_ends, j.p.ends_min_ratio, j.sym ? 1 : 0, o.counts.data(), o.status.data(), nullptr, &o.sum,
                                              &bad_index, nullptr);
    done(j, rc, bad_index, "overlap_ends");
}

// The reads overlap_ends() found contained, a byte each: the mask --best-overlaps and --string-graph leave reads out by.
std::vector<uint8_t> contained_reads(const Job &j)
{
    std::vector<uint8_t> skip(j.ends.status.size());
    for (size_t r = 0; r < skip.size(); ++r) skip[r] = j.ends.status[r] == RAFT_HIP_END_READ_CONTAINED ? 1 : 0;
    return skip;
}

// --best-overlaps: the best overlap of every read end and whether it is mutual (raft_hip_best_overlaps_host), directly behind
// overlap_ends(): on the first context over the same whole stream under the same H, F and symmetric flag, with the reads that phase
// found contained left out (their status byte is the mask).
void best_overlaps(Job &j)
{
    BestOut &o = j.best;
    o.partner.resize((size_t)j.n_reads * 2); o.span.resize((size_t)j.n_reads * 2); o.flags.resize((size_t)j.n_reads);
    const std::vector<uint8_t> skip = contained_reads(j);
    const raft_hip_records r = records(j);
    int64_t bad_index = -1;
    const int rc = raft_hip_best_overlaps_host(j.ctxs[0], j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, j.strand, skip.data(),
                                               j.p.overlap_ends, j.p.ends_min_ratio, j.sym ? 1 : 0, o.partner.data(), o.span.data(), o.flags.data(), &o.sum,
                                               &bad_index, nullptr);
    done(j, rc, bad_index, "best_overlaps");
}

// --unitigs: the chains and cycles of the mutual best overlaps (raft_hip_unitigs_host), directly behind best_overlaps() on the
// arrays that phase holds.
void unitigs(Job &j)
{
    UnitigOut &o = j.utg;
    const size_t n = (size_t)j.n_reads;
    o.unitig.resize(n); o.index.resize(n); o.order.resize(n); o.reads.resize(n);
    o.offset.resize(n); o.off.resize(n + 1); o.length.resize(n);
    o.orient.resize(n); o.circular.resize(n);
    int64_t bad_index = -1;
    const int rc = raft_hip_unitigs_host(j.ctxs[0], j.n_reads, j.rl, j.best.partner.data(), j.best.span.data(), j.best.flags.data(), o.unitig.data(),
                                         o.index.data(), o.offset.data(), o.orient.data(), o.order.data(), o.off.data(), o.reads.data(), o.length.data(),
                                         o.circular.data(), &o.sum, &bad_index, nullptr, nullptr);
    done(j, rc, bad_index, "unitigs");
}

// --components: the connected components of the graph whose edges are the containments and the dovetails (raft_hip_components_host),
// behind unitigs(): on the first context over the same whole stream as overlap_ends(), under its H and F and the job's symmetric flag.
void components(Job &j)
{
    ComponentsOut &o = j.cc;
    const size_t n = (size_t)j.n_reads;
    o.component.resize(n); o.degree.resize(n); o.first.resize(n); o.reads.resize(n); o.bases.resize(n); o.sides.resize(n);
    const raft_hip_records r = records(j);
    int64_t bad_index = -1;
    const int rc = raft_hip_components_host(j.ctxs[0], j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, j.strand,
                                            j.p.overlap_ends, j.p.ends_min_ratio, RAFT_HIP_CC_KINDS_PROPER, j.sym ? 1 : 0, o.component.data(),
                                            o.degree.data(), o.first.data(), o.reads.data(), o.bases.data(), o.sides.data(), &o.sum, &bad_index,
                                            nullptr, nullptr);
    done(j, rc, bad_index, "components");
}

// --string-graph: the dovetails between the reads that are not contained, one arc per pair of read ends, transitively reduced
// (raft_hip_string_graph_host), behind components(): on the first context over the same whole stream as overlap_ends(), under its H and
// F, the job's symmetric flag and best_overlaps()' mask.  One call where the edge list fits the first capacity (cli_plan.hpp
// string_graph_capacity0), which it does unless the graph branches at most ends; else the call says what it needs and runs once more.
void string_graph(Job &j)
{
    StringGraphOut &o = j.sg;
    const size_t n = (size_t)j.n_reads;
    o.arcs.resize(2 * n); o.kept.resize(2 * n); o.flags.resize(n);
    const std::vector<uint8_t> skip = contained_reads(j);
    const raft_hip_records r = records(j);
    int64_t bad_index = -1, n_out = 0;
    const auto call = [&](int64_t cap) {
        o.u.resize((size_t)cap); o.w.resize((size_t)cap); o.span.resize((size_t)cap);
        return raft_hip_string_graph_host(j.ctxs[0], j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, j.strand, skip.data(),
                                          j.p.overlap_ends, j.p.ends_min_ratio, j.sym ? 1 : 0, j.p.string_graph_fuzz, 0, cap, o.arcs.data(), o.kept.data(),
                                          nullptr, nullptr, o.flags.data(), o.u.data(), o.w.data(), o.span.data(), nullptr, nullptr, nullptr, &n_out,
                                          &o.sum, &bad_index, nullptr, nullptr);
    };
    int rc = call(raft_cli::string_graph_capacity0(r.n_rec, j.n_reads));
    if (rc == RAFT_HIP_ERR_TOO_LARGE && n_out > (int64_t)o.u.size()) rc = call(n_out);      // (the one refusal that names a size: out_cap below n_out)
    if (rc == RAFT_HIP_OK) { o.u.resize((size_t)n_out); o.w.resize((size_t)n_out); o.span.resize((size_t)n_out); }
    done(j, rc, bad_index, "string_graph");
}

// --containment: the forest of the contained reads (raft_hip_containment_host), behind string_graph(): on the first context over the same
// whole stream as overlap_ends(), under its H and F and the job's symmetric flag.
void containment(Job &j)
{
    ContainmentOut &o = j.ctn;
    const size_t n = (size_t)j.n_reads;
    o.parent.resize(n); o.pos.resize(n); o.span.resize(n); o.root.resize(n); o.root_pos.resize(n); o.depth.resize(n); o.children.resize(n);
    o.flags.resize(n); o.tree_reads.resize(n); o.tree_bases.resize(n);
    const raft_hip_records r = records(j);
    int64_t bad_index = -1;
    const int rc = raft_hip_containment_host(j.ctxs[0], j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, j.strand,
                                             j.p.overlap_ends, j.p.ends_min_ratio, j.sym ? 1 : 0, o.parent.data(), o.pos.data(), o.span.data(),
                                             o.root.data(), o.root_pos.data(), o.depth.data(), o.children.data(), o.flags.data(), o.tree_reads.data(),
                                             o.tree_bases.data(), nullptr, &o.sum, &bad_index, nullptr);
    done(j, rc, bad_index, "containment");
}

// ... with --unitigs: that forest on the layout unitigs() holds (raft_hip_place_contained_host), directly behind containment().
void place_contained(Job &j)
{
    PlaceOut &o = j.plc;
    const size_t n = (size_t)j.n_reads, n_utg = (size_t)j.utg.sum.unitigs;
    o.unitig.resize(n); o.start.resize(n); o.orient.resize(n); o.reads.resize(n_utg); o.bases.resize(n_utg); o.permille.resize(n_utg);
    int64_t bad_index = -1;
    const int rc = raft_hip_place_contained_host(j.ctxs[0], j.n_reads, j.rl, j.ctn.root.data(), j.ctn.root_pos.data(), j.ctn.flags.data(), j.utg.unitig.data(),
                                                 j.utg.offset.data(), j.utg.orient.data(), (int32_t)n_utg, j.utg.length.data(), o.unitig.data(),
                                                 o.start.data(), o.orient.data(), o.reads.data(), o.bases.data(), o.permille.data(), &o.sum, &bad_index,
                                                 nullptr);
    done(j, rc, bad_index, "place_contained");
}

// --graph-clean: string_graph()'s surviving edges without the weak ones and the tips (raft_hip_graph_clean_host), behind every other
// option of the stream: on the first context, under the same mask of contained reads.  The live edges are kept for the writer.
void graph_clean(Job &j)
{
    GraphCleanOut &o = j.cln;
    const StringGraphOut &g = j.sg;
    const size_t n = (size_t)j.n_reads, m = g.u.size();
    o.edge_state.resize(m); o.read_state.resize(n); o.read_round.resize(n); o.flags.resize(n);
    o.arcs.resize(2 * n); o.weak.resize(2 * n); o.kept.resize(2 * n); o.partner.resize(2 * n); o.span.resize(2 * n);
    const std::vector<uint8_t> skip = contained_reads(j);
    int64_t bad_index = -1;
    const int rc = raft_hip_graph_clean_host(j.ctxs[0], j.n_reads, j.rl, skip.data(), (int64_t)m, g.u.data(), g.w.data(), g.span.data(), j.p.clean_min_ratio,
                                             j.p.clean_tip_reads, j.p.clean_rounds, o.edge_state.data(), nullptr, o.read_state.data(), o.read_round.data(),
                                             o.arcs.data(), o.weak.data(), o.kept.data(), o.partner.data(), o.span.data(), o.flags.data(), &o.sum, &bad_index,
                                             nullptr, nullptr);
    done(j, rc, bad_index, "graph_clean");
    for (size_t e = 0; e < m; ++e)
        if (o.edge_state[e] == 0) { o.u.push_back(g.u[e]); o.w.push_back(g.w[e]); o.edge_span.push_back(g.span[e]); }
}

// ... and the unitigs of the cleaned table (raft_hip_unitigs_host), directly behind graph_clean().
void graph_clean_unitigs(Job &j)
{
    const GraphCleanOut &c = j.cln;
    UnitigOut &o = j.cln.utg;
    const size_t n = (size_t)j.n_reads;
    o.unitig.resize(n); o.index.resize(n); o.order.resize(n); o.reads.resize(n);
    o.offset.resize(n); o.off.resize(n + 1); o.length.resize(n);
    o.orient.resize(n); o.circular.resize(n);
    int64_t bad_index = -1;
    const int rc = raft_hip_unitigs_host(j.ctxs[0], j.n_reads, j.rl, c.partner.data(), c.span.data(), c.flags.data(), o.unitig.data(), o.index.data(),
                                         o.offset.data(), o.orient.data(), o.order.data(), o.off.data(), o.reads.data(), o.length.data(), o.circular.data(),
                                         &o.sum, &bad_index, nullptr, nullptr);
    done(j, rc, bad_index, "graph_clean_unitigs");
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
    if (j.rq.keep_query_ids) j.qid_kept.assign(j.col[0], j.col[0] + j.n_rec);   // (put back behind run_engine)
    if (j.prepare && j.sym && j.n_rec > 0 && !j.sw.no_grouped) {
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
    const bool few_runs = j.sym && !j.prepare && j.n_rec > 0 && raft_cli::few_sorted_runs(j.col[0], j.n_rec);
    j.cov_width = raft_cli::first_cov_width(j.n_runs, few_runs, j.sw.no_delta4, j.ranks, j.p.est_cov);
}

// upload, pass and download of consecutive read ranges overlap, on every device named (one piece for small inputs)
int call_engine(Job &j, raft_hip_host_outputs *ho)
{
    raft_hip_ctx **ctxs = j.ctxs.data();
    const int32_t n_ctx = (int32_t)j.ctxs.size();
    const raft_hip_records r = records(j, j.ranks == 0 && j.sym ? Targets::none : Targets::all);
    if (j.ranks > 0)
        return raft_hip_run_presplit_local(ctxs, n_ctx, j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, ho, &j.s);
    if (j.win)
        return raft_hip_run_multi_windows(ctxs, n_ctx, j.n_reads, j.rl, j.n_rec, j.n_runs, j.rec_off.get(), j.win, j.sw.chunks, ho, &j.s);
    if (j.n_runs > 0)
        return raft_hip_run_multi_grouped(ctxs, n_ctx, j.n_reads, j.rl, j.n_rec, j.n_runs, j.rec_off.get(), j.col[1], j.col[2], j.sw.chunks, ho, &j.s);
    return raft_hip_run_multi(ctxs, n_ctx, j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, j.sw.chunks, ho, &j.s);
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
    if (!j.qid_kept.empty()) j.col[0] = j.qid_kept.data();          // (the query ids, for the options that read them after the job)
    done(j, rc, j.s.error_index, "engine+fetch");
}

// The three on the job's results take the tokenised columns and the host arrays reads.fasta and long_repeats.txt are written from, on
// the first context: the same call whichever way the job ran (one device or several, ranks, -e auto).
// --repeat-overlaps: against the job's own repeat annotation.  Both sides are classified; the reads' tallies follow the job's
// symmetric flag, as the census does.
void repeat_overlaps(Job &j)
{
    RepeatOverlapsOut &o = j.ovl;
    o.cls.resize((size_t)j.n_rec); o.flags.resize((size_t)j.n_reads);
    o.touch.resize((size_t)j.n_reads); o.repeat.resize((size_t)j.n_reads);
    const raft_hip_records r = records(j);
    int64_t bad_index = -1;
    const int rc = raft_hip_repeat_overlaps_host(j.ctxs[0], j.n_reads, j.rl, r.n_rec, r.d_qid, r.d_qs, r.d_qe, r.d_tid, r.d_ts, r.d_te, j.sym ? 1 : 0,
                                                 j.p.min_anchor, j.rep_off[(size_t)j.n_reads], j.rep_off.data(), j.rep_s.get(), j.rep_e.get(), o.cls.data(),
                                                 o.touch.data(), o.repeat.data(), o.flags.data(), &o.sum, &bad_index, nullptr);
    done(j, rc, bad_index, "repeat_overlaps");
}

// --fragment-overlaps: against the job's own fragment rows and repeat annotation.  Sides are counted under the job's symmetric flag, as
// the census counts them.
void fragment_overlaps(Job &j)
{
    FragmentOverlapsOut &o = j.frag;
    const raft_hip_records rec = records(j);
    const raft_hip_frag_table table{j.frag_off[(size_t)j.n_reads], j.frag_off.data(), j.fb.get(), j.fe.get()};
    const raft_hip_frag_repeats repeats{j.rep_off[(size_t)j.n_reads], j.rep_off.data(), j.rep_s.get(), j.rep_e.get()};
    for (std::vector<int32_t> *v : {&o.touch, &o.span, &o.contained, &o.repeat}) v->resize((size_t)table.n_frag);
    int64_t bad_index = -1;
    const int rc = raft_hip_frag_overlaps_host(j.ctxs[0], j.n_reads, j.rl, &rec, j.sym ? 1 : 0, &table, &repeats, o.touch.data(), o.span.data(),
                                               o.contained.data(), o.repeat.data(), nullptr, &o.sum, &bad_index, nullptr);
    done(j, rc, bad_index, "fragment_overlaps");
}

// --fragment-paf: the job's kept stream lifted onto the job's own fragment rows.  A size query, the eight columns at that size, the call.
void fragment_paf(Job &j)
{
    LiftOut &o = j.lift;
    const raft_hip_records rec = records(j);
    const raft_hip_frag_table table{j.frag_off[(size_t)j.n_reads], j.frag_off.data(), j.fb.get(), j.fe.get()};
    int64_t bad_index = -1;
    int rc = raft_hip_lift_overlaps_host(j.ctxs[0], j.n_reads, &rec, j.strand, &table, j.p.fragment_paf_min, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, &o.sum, &bad_index, nullptr);
    const size_t n_out = rc == RAFT_HIP_OK ? (size_t)o.sum.n_out : 0;
    if (n_out > 0) {
        for (auto &c : o.col) c.resize(n_out);
        o.rev.resize(n_out); o.src.resize(n_out);
        rc = raft_hip_lift_overlaps_host(j.ctxs[0], j.n_reads, &rec, j.strand, &table, j.p.fragment_paf_min, (int64_t)n_out, o.col[0].data(), o.col[1].data(),
                                         o.col[2].data(), o.col[3].data(), o.col[4].data(), o.col[5].data(), o.rev.data(), o.src.data(), &o.sum, &bad_index,
                                         nullptr);
    }
    done(j, rc, bad_index, "fragment_paf");
}

// The writers of the optional outputs (-> RAFT_HOST_OK or not) and their stdout lines, in the words of cli_plan.hpp where they are there.
int write_read_stats(Job &j)
{
    return raft_host_write_read_stats((j.p.prefix + ".read_stats.tsv").c_str(), j.n_reads, names(j), j.rl, j.p.reso, j.rs.intervals.data(), j.rs.contained.data(),
                                      j.rs.sum.data(), j.rs.max.data(), j.rs.high.data(), j.rep_off.data(), j.frag_off.data());
}
std::string line_read_stats(const Job &j) { return "INFO, read_stats(), contained reads = " + std::to_string(j.rs.n_contained) + " of " + std::to_string(j.n_reads); }

int write_low_coverage(Job &j)
{
    return raft_host_write_low_coverage((j.p.prefix + ".low_coverage.bed").c_str(), j.n_reads, names(j), j.low.off.data(), j.low.s.data(), j.low.e.data(), j.rl,
                                        j.p.reso);
}
std::string line_low_coverage(const Job &j)
{
    return "INFO, low_coverage(), low_cov = " + std::to_string(j.p.low_cov) + ", runs = " + std::to_string(j.low.sum.n_runs) + ", reads with an interior run = " +
           std::to_string(j.low.sum.reads_interior) + ", uncovered reads = " + std::to_string(j.low.sum.reads_uncovered) + " of " + std::to_string(j.n_reads);
}

int write_repeat_overlaps(Job &j)
{
    return raft_host_write_repeat_overlaps((j.p.prefix + ".repeat_overlaps.tsv").c_str(), (j.p.prefix + ".repeat_overlaps.records.tsv").c_str(), j.n_reads,
                                           names(j), j.rl, j.ovl.touch.data(), j.ovl.repeat.data(), j.ovl.flags.data(), j.n_rec, j.col[0], j.col[1], j.col[2],
                                           j.col[3], j.col[4], j.col[5], j.ovl.cls.data());
}
std::string line_repeat_overlaps(const Job &j)
{
    const raft_hip_ovl_summary &s = j.ovl.sum;
    return "INFO, repeat_overlaps(), min_anchor = " + std::to_string(j.p.min_anchor) + ", records = " + std::to_string(s.n_records) +
           ", query side in a repeat = " + std::to_string(s.q_repeat) + ", target side = " + std::to_string(s.t_repeat) + ", both = " +
           std::to_string(s.both_repeat) + ", contained reads = " + std::to_string(s.reads_contained) + ", contained only inside repeats = " +
           std::to_string(s.reads_repeat_contained);
}

int write_fragment_overlaps(Job &j)
{
    return raft_host_write_fragments((j.p.prefix + ".fragments.tsv").c_str(), j.n_reads, names(j), j.frag_off.data(), j.fb.get(), j.fe.get(), j.frag.touch.data(),
                                     j.frag.span.data(), j.frag.contained.data(), j.frag.repeat.data());
}
std::string line_fragment_overlaps(const Job &j)
{
    const raft_hip_frag_summary &s = j.frag.sum;
    return raft_cli::fragment_overlaps_line(s.n_fragments, s.frags_spanned, s.frags_contained, s.frags_contained_repeat, s.reads_whole_spanned,
                                            s.reads_all_contained, j.n_reads);
}

// --repeat-stats: the file is written from the job's own runs, beside long_repeats.txt; the rows come from the stats pass, which must
// have found the same number of runs
int write_repeat_stats(Job &j)
{
    const RepeatStatsOut &o = j.rst;
    const int64_t n_rep = j.rep_off[(size_t)j.n_reads];
    if (!o.done || (int64_t)o.flags.size() != n_rep)
        die("ERROR, repeat_stats(), the stats pass found " + std::to_string(o.flags.size()) + " repeats, the job " + std::to_string(n_rep));
    return raft_host_write_repeat_stats((j.p.prefix + ".long_repeats.stats.tsv").c_str(), j.n_reads, names(j), j.rep_off.data(), j.rep_s.get(), j.rep_e.get(),
                                        o.flags.data(), o.windows.data(), o.cov_sum.data(), o.min.data(), o.max.data(), o.high.data(), o.touch.data(),
                                        o.span.data(), o.inside.data());
}
std::string line_repeat_stats(const Job &j) { const auto &s = j.rst.sum; return raft_cli::repeat_stats_line(s.n_runs, s.runs_interior, s.runs_spanned, s.interior_spanned, s.runs_touched, s.sides_inside); }

int write_overlap_ends(Job &j) { return raft_host_write_overlap_ends((j.p.prefix + ".overlap_ends.tsv").c_str(), j.reads, j.ends.counts.data(), j.ends.status.data()); }
std::string line_overlap_ends(const Job &j)
{
    const raft_hip_end_summary &s = j.ends.sum;
    return raft_cli::overlap_ends_line(j.p.overlap_ends, j.p.ends_min_ratio, s.n_records, s.kind_internal, s.kind_query_contained, s.kind_target_contained,
                                       s.kind_end3 + s.kind_end5, s.kind_self, s.kind_invalid, s.reads_contained, s.reads_dead5 + s.reads_dead3,
                                       s.reads_isolated, j.n_reads);
}

int write_best_overlaps(Job &j)
{
    return raft_host_write_best_overlaps((j.p.prefix + ".best_overlaps.tsv").c_str(), j.reads, j.best.partner.data(), j.best.span.data(), j.best.flags.data());
}
std::string line_best_overlaps(const Job &j)
{
    const raft_hip_best_summary &s = j.best.sum;
    return raft_cli::best_overlaps_line(s.n_records, s.candidates, s.left_out, s.ends_best, s.ends_mutual, s.reads_both_mutual, s.reads_no_best,
                                        s.reads_skipped, j.n_reads);
}

int write_unitigs(Job &j)
{
    const UnitigOut &o = j.utg;
    return raft_host_write_unitigs(j.p.prefix.c_str(), j.reads, o.sum.unitigs, o.unitig.data(), o.index.data(), o.offset.data(), o.orient.data(), o.order.data(),
                                   o.off.data(), o.reads.data(), o.length.data(), o.circular.data());
}
std::string line_unitigs(const Job &j)
{
    const raft_hip_utg_summary &s = j.utg.sum;
    return raft_cli::unitigs_line(s.reads_in, s.reads_skipped, s.unitigs, s.singletons, s.circular, s.longest_reads, s.longest_length, s.total_length,
                                  raft_cli::unitig_n50(j.utg.length.data(), s.unitigs));
}

int write_components(Job &j)
{
    const ComponentsOut &o = j.cc;
    return raft_host_write_components(j.p.prefix.c_str(), j.reads, o.sum.components, o.component.data(), o.degree.data(), o.first.data(), o.reads.data(),
                                      o.bases.data(), o.sides.data());
}
std::string line_components(const Job &j)
{
    const raft_hip_cc_summary &s = j.cc.sum;
    return raft_cli::components_line(RAFT_HIP_CC_KINDS_PROPER, s.n_records, s.edge_records, s.components, s.singletons, s.largest_reads, s.largest_bases,
                                     s.total_bases, s.reads_in_largest_permille, s.n_reads);
}

int write_string_graph(Job &j)
{
    const StringGraphOut &o = j.sg;
    return raft_host_write_string_graph(j.p.prefix.c_str(), j.reads, o.arcs.data(), o.kept.data(), o.flags.data(), (int64_t)o.u.size(), o.u.data(), o.w.data(),
                                        o.span.data());
}
std::string line_string_graph(const Job &j)
{
    const raft_hip_sg_summary &s = j.sg.sum;
    return raft_cli::string_graph_line(j.p.string_graph_fuzz, s.records, s.dovetail_views, s.views_left_out, s.arcs, s.duplicate_arcs, s.unpaired_arcs,
                                       s.reducible_arcs, s.edges, s.kept_edges, s.ends_kept_one, s.ends_kept_more, s.ends_dead, s.ends_mutual,
                                       s.reads_flagged, s.longest_row, j.n_reads);
}

// (the placed columns are there with --unitigs: place_contained() ran)
int write_containment(Job &j)
{
    const ContainmentOut &o = j.ctn;
    const bool placed = j.p.unitigs;
    return raft_host_write_containment((j.p.prefix + ".containment.tsv").c_str(), j.reads, o.parent.data(), o.pos.data(), o.span.data(), o.root.data(),
                                       o.root_pos.data(), o.depth.data(), o.children.data(), o.flags.data(), o.tree_reads.data(), o.tree_bases.data(),
                                       placed ? j.plc.unitig.data() : nullptr, placed ? j.plc.start.data() : nullptr, placed ? j.plc.orient.data() : nullptr);
}
std::string line_containment(const Job &j)
{
    const raft_hip_ctn_summary &s = j.ctn.sum;
    return raft_cli::containment_line(s.records, s.containment_views, s.views_not_longer, s.reads_with_parent, s.orphans, s.roots, s.roots_with_tree,
                                      s.greatest_depth, s.largest_tree_reads, s.largest_tree_bases);
}

int write_unitig_depth(Job &j)
{
    const PlaceOut &o = j.plc;
    return raft_host_write_unitig_depth((j.p.prefix + ".unitigs.depth.tsv").c_str(), j.utg.sum.unitigs, j.utg.reads.data(), j.utg.length.data(), o.reads.data(),
                                        o.bases.data(), o.permille.data());
}
std::string line_place_contained(const Job &j)
{
    const raft_hip_place_summary &s = j.plc.sum;
    return raft_cli::place_contained_line(s.n_unitigs, s.placed, s.unplaced, s.n_reads, s.unitigs_gained, s.greatest_depth_permille);
}

int write_fragment_paf(Job &j)
{
    const LiftOut &o = j.lift;
    return raft_host_write_fragment_paf((j.p.prefix + ".fragments.paf").c_str(), j.reads, j.frag_off.data(), j.fb.get(), j.fe.get(), o.sum.n_out, o.col[0].data(),
                                        o.col[1].data(), o.col[2].data(), o.col[3].data(), o.col[4].data(), o.col[5].data(), o.rev.data(), o.src.data(),
                                        j.matches, j.block);
}
std::string line_fragment_paf(const Job &j) { const auto &s = j.lift.sum; return raft_cli::fragment_paf_line(j.p.fragment_paf_min, s.n_records, s.n_out, s.records_cut, s.records_none, s.pairs_dropped, s.most_per_record); }

// PREFIX.clean.tsv, and the cleaned graph through string_graph's writer under the prefix PREFIX.clean: arcs the degrees before, kept after
int write_graph_clean(Job &j)
{
    const GraphCleanOut &o = j.cln;
    const int rc = raft_host_write_graph_clean((j.p.prefix + ".clean.tsv").c_str(), j.reads, o.read_state.data(), o.read_round.data(), o.weak.data(), o.kept.data());
    if (rc != RAFT_HOST_OK) return rc;
    return raft_host_write_string_graph((j.p.prefix + ".clean").c_str(), j.reads, o.arcs.data(), o.kept.data(), o.flags.data(), (int64_t)o.u.size(), o.u.data(),
                                        o.w.data(), o.edge_span.data());
}
std::string line_graph_clean(const Job &j)
{
    const raft_hip_cln_summary &s = j.cln.sum;
    return raft_cli::graph_clean_line(j.p.clean_min_ratio, j.p.clean_tip_reads, s.rounds_run, j.p.clean_rounds, s.converged, s.edges, s.weak_edges, s.tips,
                                      s.tip_reads, s.tip_bases, s.tip_edges, s.kept_edges, s.ends_kept_more, s.ends_dead, s.isolated_short);
}

int write_graph_clean_unitigs(Job &j)
{
    const UnitigOut &o = j.cln.utg;
    return raft_host_write_unitigs((j.p.prefix + ".clean").c_str(), j.reads, o.sum.unitigs, o.unitig.data(), o.index.data(), o.offset.data(), o.orient.data(),
                                   o.order.data(), o.off.data(), o.reads.data(), o.length.data(), o.circular.data());
}
std::string line_graph_clean_unitigs(const Job &j)
{
    const raft_hip_utg_summary &s = j.cln.utg.sum;
    return raft_cli::graph_clean_unitigs_line(s.reads_in, s.reads_skipped, s.unitigs, s.singletons, s.circular, s.longest_reads, s.longest_length,
                                              s.total_length, raft_cli::unitig_n50(j.cln.utg.length.data(), s.unitigs));
}

std::string line_filter_overlaps(const Job &j) { const auto &s = j.flt.sum; return raft_cli::filter_overlaps_line(j.p.min_identity, j.p.min_overlap, s.n_records, s.n_kept, s.below_identity, s.below_span); }

// The optional outputs, one row each, in the one order in which they run, are written and report on stdout.  name: that of the row's
// `ERROR, name(), cannot write output files`, of its stdout line and -- the census apart -- of its stage on the clock.  stage: where
// run stands in main() -- on the stream before the job (prepare_input() writes window records over the query column), on the job's
// results, or inside the survey (a phase of its own, as the filter is: it calls its three by name).  run, write and line may be null.
enum class Stage { stream, results, survey };

struct Extra { const char *name; bool (*wanted)(const Job &); Stage stage; void (*run)(Job &); int (*write)(Job &); std::string (*line)(const Job &); };

const Extra kExtras[] = {
    {"filter_overlaps", [](const Job &j) { return j.rq.filter; }, Stage::stream, nullptr, nullptr, line_filter_overlaps},
    {"read_stats", [](const Job &j) { return j.p.read_stats; }, Stage::stream, census, write_read_stats, line_read_stats},
    {"low_coverage", [](const Job &j) { return j.p.low_cov >= 0; }, Stage::survey, nullptr, write_low_coverage, line_low_coverage},
    {"repeat_overlaps", [](const Job &j) { return j.p.min_anchor > 0; }, Stage::results, repeat_overlaps, write_repeat_overlaps, line_repeat_overlaps},
    {"fragment_overlaps", [](const Job &j) { return j.p.fragment_overlaps; }, Stage::results, fragment_overlaps, write_fragment_overlaps, line_fragment_overlaps},
    {"repeat_stats", [](const Job &j) { return j.p.repeat_stats; }, Stage::survey, nullptr, write_repeat_stats, line_repeat_stats},
    {"overlap_ends", [](const Job &j) { return j.p.overlap_ends >= 0; }, Stage::stream, overlap_ends, write_overlap_ends, line_overlap_ends},
    {"best_overlaps", [](const Job &j) { return j.p.best_overlaps; }, Stage::stream, best_overlaps, write_best_overlaps, line_best_overlaps},
    {"unitigs", [](const Job &j) { return j.p.unitigs; }, Stage::stream, unitigs, write_unitigs, line_unitigs},
    {"components", [](const Job &j) { return j.p.components; }, Stage::stream, components, write_components, line_components},
    {"string_graph", [](const Job &j) { return j.p.string_graph; }, Stage::stream, string_graph, write_string_graph, line_string_graph},
    {"containment", [](const Job &j) { return j.p.containment; }, Stage::stream, containment, write_containment, line_containment},
    {"place_contained", [](const Job &j) { return j.p.containment && j.p.unitigs; }, Stage::stream, place_contained, write_unitig_depth, line_place_contained},
    {"fragment_paf", [](const Job &j) { return j.p.fragment_paf; }, Stage::results, fragment_paf, write_fragment_paf, line_fragment_paf},
    {"graph_clean", [](const Job &j) { return j.p.graph_clean; }, Stage::stream, graph_clean, write_graph_clean, line_graph_clean},
    {"graph_clean_unitigs", [](const Job &j) { return j.p.graph_clean; }, Stage::stream, graph_clean_unitigs, write_graph_clean_unitigs, line_graph_clean_unitigs},
};

void run_extras(Job &j, Stage stage)
{
    for (const Extra &e : kExtras)
        if (e.stage == stage && e.run && e.wanted(j)) e.run(j);
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

// the four output files are independent: the FASTA is written beside the coverage/repeat tables
void write_outputs(Job &j)
{
    const Options &p = j.p;
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
    for (const Extra &e : kExtras)
        if (e.write && e.wanted(j) && e.write(j) != RAFT_HOST_OK) die(std::string("ERROR, ") + e.name + "(), cannot write output files");
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
    for (const Extra &e : kExtras)
        if (e.line && e.wanted(j)) std::cout << e.line(j) << "\n";
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
    run_extras(job, Stage::stream);
    prepare_input(job);
    lock_inputs(job);
    choose_encoding(job);
    run_engine(job);
    run_extras(job, Stage::results);
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
