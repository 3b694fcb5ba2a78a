// engine_ctx.hpp -- what the engine's translation units share: the context (one device + its streams and grow-only buffers), the
// device buffers with their placement (virtual ranges over pooled 32 MiB chunks), the control block, error plumbing.
//   engine.hip            context life cycle, one pass (run_pass), finish / fetch / encodings -- and every kernel header.
//                         run_pass is a sequence of phases over one plain PassPlan: read_switches, resolve_input, reset_and_decide,
//                         open_pass, find_sizes, choose_quantum, ensure_buffers, launch_head, decide_source, fill_pileup_args,
//                         interval_source (bucket_sides), launch_pileup, launch_tail; raft_hip_finish is wait_for_pass, rerun_ladder,
//                         collect_summary
//   engine_pipeline.hip   the host-to-host entry points: chunked upload / pass / download, several contexts, routed streams
//                         run_multi_impl is a sequence of phases over one plain PipelinePlan: check_arguments, choose_route, decide_derive,
//                         plan_chunks, place_jobs, prepare_contexts, make_rings, run_lanes (Lane: a method per stage of a chunk),
//                         drain_and_collect, reorder_exceptions, close_gaps
//   pipeline_plan.hpp     its arithmetic, free of HIP: WindowDiv, the sorted runs, the chunk plan, the jobs' places, derive_slice
//   engine_exchange.hip   pre-split PAF: symmetric flag across ranks, grouped sides, the exchange (RCCL / peer copies), the pre-split job
//   engine_placement.hip  where buffers lie: pool, trim, policy, the placement trial, the callers' input buffers, page-locking
//   query_host.hpp        the host side the queries about a finished pass or a record stream share (engine.hip's and the *_lib.hip libraries'):
//                         phases, copy tables, staging of a host form, the event pair, the control words
//   query_args.hpp        their decisions about arguments, free of HIP; cov_decode.hpp: the coverage decoded to int32, one launch sequence
#pragma once
#include "../../include/raft_hip.h"
#include "raft_types.hpp"
#include "wave_launch.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <utility>
#include <vector>

namespace raft {

// The windows of a wave tile (pileup_wave.hpp): its LDS array minus three alignment slots and the sentinel.  A read with more
// windows is piled up in pieces of that many (joined by finalize_count_kernel).
constexpr int kTileCap = kWaveSlots - 4;
constexpr int kWaveCounters = 32;      // tile hand-out counters of the wave kernel, 256 bytes apart (pileup_wave.hpp next_range)
constexpr int kWinMaxRuns = 2;         // runs the window-record instantiations (pileup_wave.hpp IN = 1) take; more: unpacked to coordinate columns first
// coverage arrays a context's placement trial compares (placement_trial): off unless asked for -- RAFT_PLACEMENT_TRIALS=<k>, k >= 2, or
// raft_hip_set_placement_trial
inline int default_trial_candidates()
{
    static const int v = [] { const char *e = getenv("RAFT_PLACEMENT_TRIALS"); return e ? std::max(0, std::min(8, atoi(e))) : 0; }();
    return v;
}

struct Ctrl {                         // device control block, cleared every pass
    int32_t err_flags;
    int32_t pad_slow;
    long long err_index;              // (the first 16 bytes are what the pass's host wait reads back)
    int32_t next_tile;                // (unused since round 6: the wave kernel's hand-out counters are raft_hip_ctx::wave_ctr)
    int32_t slow_next;                // delta4: the counter tile ids are drawn from (PileupArgs::slow_counter)
    int32_t pad_extra[2];
    unsigned long long totals[4];     // coverage, repeat bp, read length
    InspectOut insp;
    long long out_totals[4];          // rep / cut / frag totals land here via the scan
    GuessOut guess;                   // sorted runs as seen from samples
    unsigned long long n_exc;         // windows at or above the limit of the encoding a pass wrote directly (PileupArgs::n_exc)
    int32_t n_deep, pad_deep;         // tiles pileup_wave_kernel listed for pileup_deep_kernel (may exceed the list: kErrDeep)
};

// Device buffers.  The large ones the pass streams through (coverage, repeats, cut points, fragments, the pipeline's staging
// columns: `big`) are virtual ranges over 32 MiB physical chunks (hipMemCreate / hipMemMap) that are SPREAD over a wide
// physical span: for a buffer of 1 GiB or more eight times the chunks are created and every eighth is mapped, in a
// shuffled order.
// Why (tools/membench, profiles/r04_membench_placement.txt; tools/placement_probe2.py): what a stream gets from this part
// is a property of where its buffer lies.  Plain stores into an 8 GB hipMalloc block: 5.65 TB/s, with few exceptions; into
// chunks taken one after the other: 5.6 .. 7.1 TB/s from buffer to buffer; into every eighth chunk of a 64 GB span:
// 7.0 .. 7.1 TB/s, every time.  The pileup kernel followed its coverage array -- contexts of ONE process ran at 2.14 or at
// 2.6 ms, and swapping their `cov` buffers swapped their times.
// Two rules the mapping calls turned out to need on this stack (tools/gpu_tmp.py's sequence: one-byte coverage, then two-byte
// coverage in the same context -- tests/test_gpu_windows.py):
//   * a virtual range is reserved once and never given back (hipMemAddressFree) while the process lives.  A range that was
//     unmapped, freed and handed out again by the next hipMemAddressReserve was served from STALE translations: writes and reads
//     of the new buffer went to the chunks the old buffer had been mapped to, deterministically from the second chunk on.
//     (Address space is not scarce: 47 bits.  A range never mapped -- a failed attempt -- may go back.)
//   * chunks are not handed back to the driver either: the spare ones, and the ones of a buffer that is released or outgrown,
//     go to a per-device pool that later buffers draw from (random picks: spread again) -- no create / release storm when a
//     buffer grows, and nothing depends on when the driver wipes released memory.  Cost: the pool keeps up to seven times the
//     largest spread buffer (56 GB for the bench set's coverage array, of 288).
// Any failure falls back (fewer spare chunks, then hipMalloc); RAFT_NO_VMM=1 switches the mapping off.  Buffers other devices
// write into (the exchange's receive side) stay with hipMalloc.
struct ChunkPool {                    // per device; handles of 32 MiB physical chunks nobody maps at the moment
    std::mutex mu;
    std::vector<hipMemGenericAllocationHandle_t> free_chunks;
    unsigned long long rng = 0x9E3779B97F4A7C15ull;
    int live_ctx = 0;                 // contexts of this device: the last one to go hands the pool back to the driver
    static ChunkPool &of(int dev) { static ChunkPool pools[64]; return pools[dev & 63]; }
    unsigned long long next() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return rng >> 33; }
    // most chunks the pool keeps (RAFT_VMM_POOL_GB, default 64): what comes back beyond that goes to the driver
    static size_t cap_chunks()
    {
        static const size_t v = [] {
            const char *e = getenv("RAFT_VMM_POOL_GB");
            const double gb = e ? std::max(0.0, atof(e)) : 64.0;
            return (size_t)(gb * 32.0);                    // 32 chunks of 32 MiB per GiB
        }();
        return v;
    }
    // (mu held) a chunk nobody maps: kept for later buffers while there is room, else released
    void put(hipMemGenericAllocationHandle_t h)
    {
        if (free_chunks.size() < cap_chunks()) free_chunks.push_back(h);
        else (void)hipMemRelease(h);
    }
    // hands all but `keep` chunks back to the driver; returns how many went
    size_t trim(size_t keep)
    {
        std::lock_guard<std::mutex> lk(mu);
        size_t n = 0;
        while (free_chunks.size() > keep) { (void)hipMemRelease(free_chunks.back()); free_chunks.pop_back(); ++n; }
        if (free_chunks.empty()) free_chunks.shrink_to_fit();
        return n;
    }
};

// The streams whose work may still use a buffer this thread is about to release or re-map (the context's own and its side
// stream): release() waits for those instead of the whole device -- other contexts' passes go on.  None named: the device.
struct SyncScope {
    static inline thread_local hipStream_t streams[2] = {nullptr, nullptr};
    static inline thread_local int n = 0;
    int saved_n; hipStream_t saved[2];
    SyncScope(hipStream_t a, hipStream_t b) { saved_n = n; saved[0] = streams[0]; saved[1] = streams[1]; streams[0] = a; streams[1] = b; n = 2; }
    ~SyncScope() { n = saved_n; streams[0] = saved[0]; streams[1] = saved[1]; }
    static void wait()
    {
        if (n == 0) { (void)hipDeviceSynchronize(); return; }
        for (int i = 0; i < n; ++i) (void)hipStreamSynchronize(streams[i]);
    }
};

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool big = false;                 // may be backed by pooled chunks
    static constexpr bool kBig = true;
    DevBuf() = default;
    // a context's buffer says so where it is declared: raft_hip_destroy releases what the list names.  (Only the declared object is
    // on the list: copies and swaps move contents, `big` with them, and leave the list alone.)
    explicit DevBuf(std::vector<DevBuf *> &owner, bool big_ = false) : big(big_) { owner.push_back(this); }
    int dev = 0;                      // device of the chunks
    std::vector<hipMemGenericAllocationHandle_t> chunks;
    std::vector<size_t> map_order;    // chunk mapped at the i-th 32 MiB of the range
    size_t va_bytes = 0;
    static constexpr size_t kChunk = 32u << 20, kVmmMin = 64u << 20, kSpreadMin = size_t(1) << 30;
    // the placement policy of buffers made from now on (process-wide): 0 = plain hipMalloc, k >= 1 = chunks, k times as many made
    // as used for buffers of 1 GiB or more.  RAFT_NO_VMM=1 / RAFT_VMM_SPREAD=<k> set the start value; raft_hip_set_placement changes it.
    // set once the policy was chosen by hand (RAFT_NO_VMM / RAFT_VMM_SPREAD / raft_hip_set_placement): no placement trial then
    static std::atomic<bool> &policy_explicit()
    {
        static std::atomic<bool> e{getenv("RAFT_NO_VMM") != nullptr || getenv("RAFT_VMM_SPREAD") != nullptr};
        return e;
    }
    static std::atomic<int> &policy()
    {
        static std::atomic<int> p{getenv("RAFT_NO_VMM") ? 0 : (getenv("RAFT_VMM_SPREAD") ? std::max(1, atoi(getenv("RAFT_VMM_SPREAD"))) : 8)};
        return p;
    }
    bool map_chunks(size_t want)
    {
        const int pol = policy().load();
        if (pol <= 0) return false;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = dev;
        size_t gran = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || gran == 0 || kChunk % gran) {
            (void)hipGetLastError(); return false;
        }
        const size_t n = (want + kChunk - 1) / kChunk;
        const size_t kSpread = (size_t)pol;
        hipDeviceptr_t va = nullptr;
        if (hipMemAddressReserve(&va, n * kChunk, 0, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
        ChunkPool &pool = ChunkPool::of(dev);
        chunks.clear();
        {
            std::lock_guard<std::mutex> lk(pool.mu);
            // (1) from the pool: random picks -- its chunks lie all over the spans earlier buffers were spread over
            auto draw = [&]() {
                while (chunks.size() < n && !pool.free_chunks.empty()) {
                    const size_t j = (size_t)(pool.next() % pool.free_chunks.size());
                    chunks.push_back(pool.free_chunks[j]);
                    pool.free_chunks[j] = pool.free_chunks.back();
                    pool.free_chunks.pop_back();
                }
            };
            draw();
            // (2) the rest fresh from the driver: k times as many, every k-th for this buffer, the others into the pool; when the
            // device cannot give that many, what was made goes to the pool, serves first, and the rest is tried with fewer spares
            for (size_t k = want >= kSpreadMin ? kSpread : 1; chunks.size() < n; k /= 2) {
                const size_t need = n - chunks.size();
                if (k > 1) {
                    // spares only while the pool has room for them and the device keeps an eighth of its memory (8 GiB at least)
                    // free behind them: plain hipMalloc buffers of this pass, RCCL, torch and other processes live there
                    size_t free_b = 0, total_b = 0;
                    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; total_b = 0; }
                    const size_t reserve = std::max<size_t>(size_t(8) << 30, total_b / 8);
                    const size_t room_mem = free_b > reserve + need * kChunk ? (free_b - reserve - need * kChunk) / kChunk : 0;
                    const size_t room_pool = pool.free_chunks.size() < ChunkPool::cap_chunks() ? ChunkPool::cap_chunks() - pool.free_chunks.size() : 0;
                    const size_t spares = std::min(room_mem, room_pool);
                    while (k > 1 && need * (k - 1) > spares) k /= 2;
                }
                std::vector<hipMemGenericAllocationHandle_t> all(need * k);
                size_t made = 0;
                bool ok = true;
                for (; ok && made < need * k; ++made) ok = hipMemCreate(&all[made], kChunk, &prop, 0) == hipSuccess;
                if (!ok) { --made; (void)hipGetLastError(); }
                for (size_t i = 0; i < made; ++i) {
                    if (ok && i % k == 0) chunks.push_back(all[i]);
                    else if (ok) pool.put(all[i]);                 // spares: kept while the pool has room, else handed back
                    else pool.free_chunks.push_back(all[i]);       // (the device ran out: drawn from again right below, whatever the cap)
                }
                if (!ok) { draw(); if (k == 1) break; }
            }
            if (chunks.size() != n) {
                for (auto &h : chunks) pool.put(h);
                chunks.clear();
            }
        }
        if (chunks.size() != n) { (void)hipMemAddressFree(va, n * kChunk); return false; }
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; ++i) order[i] = i;
        unsigned long long x = 0x9E3779B97F4A7C15ull;                     // (Fisher-Yates with a fixed generator)
        for (size_t i = n; i > 1; --i) { x = x * 6364136223846793005ull + 1442695040888963407ull; std::swap(order[i - 1], order[(size_t)((x >> 33) % i)]); }
        size_t mapped = 0;
        bool ok = true;
        for (; ok && mapped < n; ++mapped) ok = hipMemMap((hipDeviceptr_t)((char *)va + mapped * kChunk), kChunk, 0, chunks[order[mapped]], 0) == hipSuccess;
        if (!ok) --mapped;
        if (ok) {
            hipMemAccessDesc acc{};
            acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
            ok = hipMemSetAccess(va, n * kChunk, &acc, 1) == hipSuccess;
        }
        if (!ok) {
            (void)hipGetLastError();
            for (size_t i = 0; i < mapped; ++i) (void)hipMemUnmap((hipDeviceptr_t)((char *)va + i * kChunk), kChunk);
            { std::lock_guard<std::mutex> lk(pool.mu); for (auto &h : chunks) pool.put(h); }
            chunks.clear();
            return false;                                  // (a range that was mapped, even in part, stays reserved)
        }
        map_order = order;
        p = va; cap = n * kChunk; va_bytes = n * kChunk;
        return true;
    }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap && p) return hipSuccess;
        release();
        size_t want = (bytes + 255) & ~size_t(255);
        if (want == 0) want = 256;
        if (big && want >= kVmmMin && map_chunks(want)) return hipSuccess;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            // out of memory with chunks parked in the pool: they go back to the driver and the request is made once more
            (void)hipGetLastError();
            int d = 0;
            if (hipGetDevice(&d) == hipSuccess && ChunkPool::of(d).trim(0) > 0) {
                if (big && want >= kVmmMin && map_chunks(want)) return hipSuccess;
                e = hipMalloc(&p, want);
            }
        }
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
    void release()
    {
        if (p && va_bytes) {
            SyncScope::wait();                             // (nothing in flight may still use the range)
            // chunk by chunk, as it was mapped; a chunk whose mapping did not go away is neither pooled nor released
            ChunkPool &pool = ChunkPool::of(dev);
            std::lock_guard<std::mutex> lk(pool.mu);
            for (size_t i = 0; i < chunks.size(); ++i) {
                if (hipMemUnmap((hipDeviceptr_t)((char *)p + i * kChunk), kChunk) == hipSuccess) pool.put(chunks[i < map_order.size() ? map_order[i] : i]);
                else (void)hipGetLastError();
            }
            // (the range stays reserved: see above)
            chunks.clear(); map_order.clear();
        } else if (p) (void)hipFree(p);
        p = nullptr; cap = 0; va_bytes = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// N buffers of a context declared as one: each is on the list like a DevBuf declared alone
template <int N> struct DevBufSet {
    DevBuf b[N];
    explicit DevBufSet(std::vector<DevBuf *> &owner) { for (DevBuf &x : b) owner.push_back(&x); }
    DevBuf &operator[](int k) { return b[k]; }
};
constexpr int kSgBufs = 40;           // the buffers of raft_hip_string_graph_* (string_graph_lib.hip SgBuf)
constexpr int kCtnBufs = 16;          // the buffers of raft_hip_containment_* and raft_hip_place_contained_* (containment_lib.hip CtnBuf)
constexpr int kClnBufs = 29;         // the buffers of raft_hip_graph_clean_* (graph_clean_lib.hip ClnBuf)

} // namespace raft

using namespace raft;

struct raft_hip_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t side_stream = nullptr;   // the per-read geometry scan of a pass that waits for its sizes runs here, beside the look at the records (find_sizes)
    bool counted = false;                // this context is one of ChunkPool::live_ctx
    hipEvent_t ev_ifork = nullptr, ev_gjoin = nullptr;   // ... forked from the main stream and joined to it
    raft_hip_params prm{};
    int32_t high_cov = 0, div = 0, minbins = 1;
    int32_t tile_q = 0;               // 0 = variant default
    int32_t force_bucket = 0;
    bool no_bucket_win = false;       // general bucketing: a side's windows did not fit 16 bits once (kErrWide): coordinate pairs from then on
    size_t cov_trial_cap = 0;         // capacity of `cov` the placement trial has been run for (placement_trial)
    double trial_ms[2] = {0.0, 0.0};  // that trial: the pileup kernel into `cov` as first placed / into the best of the other candidates (ms)
    int32_t trial_kept = 0;           // 0: the first placement stayed, 1: a plain hipMalloc block was kept, 2: another chunk mapping
    int32_t trial_candidates = default_trial_candidates();   // coverage arrays the placement trial compares; < 2: no trial (the default)
    std::string last_error;

    // device buffers: each is declared with the list (`bufs`: what raft_hip_destroy releases) and, where a pass streams through
    // it, as kBig (see DevBuf) -- the one place that names a context's buffers
    std::vector<DevBuf *> bufs;
    DevBuf len_seen{bufs};            // the read lengths as the last geometry scan saw them (see geom_id below)
    DevBuf deep_list{bufs};           // tiles too deep for 16-bit coverage (pileup_deep.hpp)
    long long deep_cap = 1024;        // its entries; grows when a pass lists more (raft_hip_finish)
    DevBuf tail_buf{bufs};            // the fused tail's sums (finalize.hpp FinalizeArgs::tail_part ...)
    DevBuf wave_ctr{bufs}, ctrl{bufs}, scan_tmp{bufs}, cov_off{bufs}, rep_res_off{bufs}, tile_first{bufs}, tile_cuts{bufs}, block_sums{bufs};
    DevBuf cov{bufs, DevBuf::kBig}, rep_cnt{bufs}, raw_key{bufs, DevBuf::kBig}, raw_s{bufs, DevBuf::kBig}, raw_e{bufs, DevBuf::kBig}, cut_cnt{bufs}, frag_cnt{bufs};
    DevBuf rep_off{bufs}, cut_off{bufs}, frag_off{bufs};
    DevBuf rep_s{bufs, DevBuf::kBig}, rep_e{bufs, DevBuf::kBig}, cuts{bufs, DevBuf::kBig};
    DevBuf frag_read{bufs, DevBuf::kBig}, frag_begin{bufs, DevBuf::kBig}, frag_end{bufs, DevBuf::kBig};
    DevBuf b_cnt{bufs}, b_off{bufs}, b_rid{bufs, DevBuf::kBig}, b_s{bufs, DevBuf::kBig}, b_e{bufs, DevBuf::kBig};
    DevBuf gs_rid{bufs, DevBuf::kBig}, gs_s{bufs, DevBuf::kBig}, gs_e{bufs, DevBuf::kBig}, gs_off{bufs}, gs_err{bufs};  // raft_hip_group_sides: the slice it hands back (+ its error word)
    std::vector<long long> gs_off_host;
    long long gs_err_index = -1;      // raft_hip_group_sides: the record (index into the slice) its last RAFT_HIP_ERR_READ_ID named
    // general streams, large inputs: (read id, start | end << 32) per side, before and after the radix sort; long runs of reads without intervals
    DevBuf rs_k0{bufs, DevBuf::kBig}, rs_k1{bufs, DevBuf::kBig}, rs_v0{bufs, DevBuf::kBig}, rs_v1{bufs, DevBuf::kBig}, gaps{bufs};
    DevBuf in_len{bufs};              // staging for raft_hip_run_host: the read lengths (the columns: in_col below)
    DevBuf samples{bufs};             // up to kSamples + 2 read ids at evenly spaced records (guess_runs_kernel): coarse index
    hipEvent_t ev_hist0 = nullptr, ev_hist1 = nullptr;   // ... and the events around its launches (made at the first call that asks for the time)
    int packed_width = 0;             // width (bytes per window) of the encoding the buffers hold, 0 = none
    long long n_exc = 0, exc_cap = 0;
    int out_width = 4;                // raft_hip_set_output_width: 1 / 2 = the pass writes the encoding, cov[] only on request
    int pass_width = 4;               // what the last pass wrote
    bool cov_valid = false;           // c->cov holds the int32 array of the last pass
    void *pinned = nullptr;           // small pinned scratch for readbacks
    long long *pinned_dev = nullptr;  // the same block as the device addresses it
    hipEvent_t ev_pass0 = nullptr, ev_pass1 = nullptr, ev_pile0 = nullptr, ev_pile1 = nullptr;

    // chunked host pipeline (raft_hip_run_pipelined): sub-contexts on the same device, one upload stream
    std::vector<raft_hip_ctx *> lanes;
    hipStream_t up_stream = nullptr, down_stream = nullptr;
    std::vector<hipEvent_t> lane_up_ev, lane_down_ev;

    // a pass that verifies in its kernels (see run_pass), and the arguments to run it again if a kernel objects
    bool spec = false;
    bool assume_sym = true;            // what a detecting context's verified pass assumes (the last detection's answer)
    // grp_*: the grouped form (raft_hip_run_device_grouped): per-run record offsets instead of searches; hint_bins >= 0: the
    // caller's window count, which sizes the pass without a host wait
    struct PassArgs {
        int32_t n_reads; const int32_t *len; int64_t n_rec; const int32_t *col[6];
        int32_t n_runs; const long long *rec_off; long long adj[kMaxSeg]; long long hint_bins;
        const uint32_t *win;           // window records instead of col[1..2] (raft_hip_run_device_windows); grouped only
    } args{};
    bool grouped = false;              // the last pass was built on the caller's offsets (verified in its kernels)
    bool no_wait = false;              // ... and sized by the caller's window count: nothing was read back on the way
    DevBuf exp_qid{bufs, DevBuf::kBig}, in_off{bufs};   // grouped input without a query column: the ids rebuilt from the offsets; staged offsets
    DevBuf m_off{bufs};                // grouped input of more than kMaxSeg runs: offsets of the merged run
    DevBuf u_s{bufs, DevBuf::kBig}, u_e{bufs, DevBuf::kBig};   // window records unpacked for the passes that need coordinate columns
    DevBuf cov_anchor{bufs}, abs_bits{bufs};   // delta4 encoding of cov[] (pack.hpp): block anchors; escape flags of the device-side decoder
    DevBuf exc_idx2{bufs}, exc_val2{bufs}, sort_tmp{bufs};   // the exception list in ascending order (sort_exceptions)
    DevBuf exc_pidx{bufs}, exc_pval{bufs}, exc_tile_n{bufs};   // delta4: the windows each tile lists, kExcPerTile slots per tile (compact_exceptions_kernel)
    bool exc_sorted = false;
    long long sizes_seq = 0;           // number of the last sizes hand-over of run_pass (publish_sizes_kernel)
    long long pass_seq = 0;            // number of the pass whose closing kernel is queued (written behind the control block when it is through)
    bool seq_armed = false;
    int d4_shift = 0;                  // delta4 on a chunk of a larger array (the host pipelines' lanes): windows of the block its first window lies in that precede it
    DevBuf x_qs{bufs}, x_qe{bufs}, x_off{bufs}, x_raw{bufs}, x_send_off{bufs}, x_cnt{bufs};   // pre-split exchange (raft_hip_exchange*): what this rank received / staged
    DevBuf cov8{bufs, DevBuf::kBig}, exc_idx{bufs}, exc_val{bufs}, exc_cnt{bufs};   // transfer encoding of cov[] (raft_hip_fetch_packed)
    DevBuf cov_hist{bufs};             // raft_hip_cov_histogram: RAFT_HIP_COV_HIST_BINS 64-bit counts, cleared at every call
    DevBuf rs_sum{bufs}, rs_max{bufs}, rs_high{bufs};   // raft_hip_read_stats: one value per read each, cleared at every call
    // The queries beside the engine (libraft_hip_low.so, _ovl.so, _frag.so, _rst.so, _flt.so, _end.so, _best.so, _utg.so; all plain allocations: those libraries keep no chunk
    // pool) share what none of them keeps between calls.  q_len, q_col, q_csr_a, q_csr_b: the staging of a host form -- lengths, the six
    // columns, the three arrays of a table the caller gave (repeat_overlaps, repeat_stats: the repeats in q_csr_a; fragment_overlaps:
    // the fragment table in q_csr_a, the repeats in q_csr_b).  q_cov, q_abs: for a pass that holds no int32 array where a query needs
    // one, the decoded coverage and delta4's escape flags (cov_decode.hpp).  One set is sound because every query call ends in a wait
    // for the stream before it returns, and a context is used by one caller at a time: no call finds another's input still in use.
    // The working and output buffers below are each query's own.
    DevBuf q_len{bufs}, q_cov{bufs}, q_abs{bufs};
    DevBuf q_col[6] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    DevBuf q_csr_a[3] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}}, q_csr_b[3] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    // raft_hip_low_coverage (low_cov_lib.hip): the two bitmaps (low windows, first windows of reads), run starts per tile and their
    // prefix, the control words; per read low windows / low bases / class bits, the flag bytes, low_offset; per run start, end and read
    DevBuf lc_bad{bufs}, lc_rs{bufs}, lc_tile_cnt{bufs}, lc_tile_base{bufs}, lc_ctl{bufs};
    DevBuf lc_win{bufs}, lc_bases{bufs}, lc_flagw{bufs}, lc_flags{bufs}, lc_off{bufs};
    DevBuf lc_s{bufs}, lc_e{bufs}, lc_read{bufs};
    // raft_hip_repeat_overlaps_* (ovl_class_lib.hip): the digest of every read's runs, per read the sides that touch / lie in a repeat
    // (one word for both while they are counted: oc_tally) and the flag words, the flags as bytes, the control words, the class bytes
    // before they go to the caller
    DevBuf oc_digest{bufs}, oc_tally{bufs}, oc_touch{bufs}, oc_repeat{bufs}, oc_flagw{bufs}, oc_flags{bufs}, oc_ctl{bufs}, oc_cls{bufs};
    // raft_hip_frag_overlaps_* (frag_ovl_lib.hip): the digest of every read's rows and of its runs, the reads' whole-spanned flag words
    // and contained rows, the difference slots (n_frag + 1), per row touch / span / contained / repeat bases, the scan's partial sums,
    // the control words
    DevBuf fo_digest{bufs}, fo_rep_digest{bufs}, fo_whole{bufs}, fo_read{bufs}, fo_slot{bufs}, fo_scan{bufs}, fo_ctl{bufs};
    DevBuf fo_out[4] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    // raft_hip_repeat_stats_* (repeat_stats_lib.hip; rst_ and not rs_: raft_hip_read_stats and the radix sort hold those names): the
    // digest of every read's runs, the read of every run, the counter slots, the control words; per run touch / span / inside,
    // windows / min / max / high windows, the coverage sum, the flag bytes
    DevBuf rst_digest{bufs}, rst_run_read{bufs}, rst_slot{bufs}, rst_ctl{bufs}, rst_sum{bufs}, rst_flags{bufs};
    DevBuf rst_cnt[3] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    DevBuf rst_win[4] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    // raft_hip_filter_overlaps_* (filter_lib.hip): the keep bitmap, the kept records of every tile and their prefix, the scan's partial
    // sums, the control words; the host form's staging of PAF columns 10 and 11 (the six columns: q_col) and the kept columns before
    // they go to the caller
    DevBuf fl_bits{bufs}, fl_tile_cnt{bufs}, fl_tile_base{bufs}, fl_scan{bufs}, fl_ctl{bufs};
    DevBuf fl_quality[2] = {DevBuf{bufs}, DevBuf{bufs}};
    DevBuf fl_out[6] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    // raft_hip_overlap_ends_* (ovl_ends_lib.hip): the five counts of every read, the status bytes, the control words; the host form's
    // staging of the strand bytes (lengths and columns: q_len, q_col) and the kind bytes before they go to the caller
    DevBuf en_cnt{bufs}, en_status{bufs}, en_ctl{bufs}, en_strand{bufs}, en_kinds{bufs};
    // raft_hip_best_overlaps_* (best_ovl_lib.hip): len | skipped << 31 of every read, the table of keys (two 64-bit slots per read), what
    // the pairs kernel writes (partner, span, the flag bytes), the control words; the host form's staging of the strand and the skip bytes
    DevBuf bo_dig{bufs}, bo_tab{bufs}, bo_partner{bufs}, bo_span{bufs}, bo_flags{bufs}, bo_ctl{bufs}, bo_strand{bufs}, bo_skip{bufs};
    // raft_hip_unitigs_* (unitig_lib.hip): the two halves of the ranking's state (32 B per half-edge each), the cycles' start reads, per
    // read {start read, index, unitig size if it is a start} / offset / the start's length / orientation, the scan's two prefix arrays
    // and partial sums, what goes to the caller (unitig, order; utg_off, utg_reads, utg_length, utg_circular), the control words; the
    // host form's staging of the flag bytes (lengths: q_len; partner and span: q_col[0], q_col[1])
    DevBuf ut_state{bufs}, ut_cut{bufs}, ut_read{bufs}, ut_offset{bufs}, ut_ulen{bufs}, ut_orient{bufs}, ut_scan{bufs}, ut_unitig{bufs}, ut_order{bufs};
    DevBuf ut_utg[4] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    DevBuf ut_ctl{bufs}, ut_flags{bufs};
    // raft_hip_lift_overlaps_* (lift_lib.hip): the digest of every read's rows, the outputs of every tile and of every lane, the tiles' prefix, the scan's
    // partial sums, the control words; the host form's staging of the strand bytes (columns and table: q_col, q_csr_a) and the eight
    // output columns before they go to the caller
    DevBuf lf_digest{bufs}, lf_tile_cnt{bufs}, lf_lane_cnt{bufs}, lf_tile_base{bufs}, lf_scan{bufs}, lf_ctl{bufs}, lf_strand{bufs};
    DevBuf lf_out[8] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    // raft_hip_components_* (components_lib.hip): the union-find's parent of every read, its root once the tree is flat, its degree, the
    // per-root accumulators (reads, then bases and sides), the roots' prefix with the scan's partial sums, what goes to the caller (the
    // component of every read; first, reads, bases, sides of every component), the control words; the host form's staging of the strand
    // bytes (lengths and columns: q_len, q_col)
    DevBuf cc_parent{bufs}, cc_root{bufs}, cc_degree{bufs}, cc_acc{bufs}, cc_scan{bufs}, cc_comp{bufs}, cc_ctl{bufs}, cc_strand{bufs};
    DevBuf cc_rows[4] = {DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}, DevBuf{bufs}};
    // raft_hip_string_graph_* (string_graph_lib.hip): one entry for all of its buffers -- the digests, the view bits and the steps'
    // offsets, the items and the sort's pairs, the chosen arcs with their rows, flags and states, the per-node tables, what goes to
    // the caller, the control words, the host form's staging of strand and skip; string_graph_lib.hip names them (SgBuf)
    DevBufSet<kSgBufs> sg{bufs};
    // raft_hip_containment_* and raft_hip_place_contained_* (containment_lib.hip): one entry for all of their buffers -- the two key
    // slots with the flag words, the children and the per-root accumulators, the two halves of the pointer jumping's state, what goes
    // to the caller, the control words, the host forms' staging; containment_lib.hip names them (CtnBuf)
    DevBufSet<kCtnBufs> ctn{bufs};
    // raft_hip_graph_clean_* (graph_clean_lib.hip): one entry for all of its buffers -- the items and the sort's pairs, the arcs with
    // their rows and live bytes, the per-node and per-read tables, the two halves of the ranking's state, the chain records, what
    // goes to the caller, the control words, the host form's staging of skip; graph_clean_lib.hip names them (ClnBuf)
    DevBufSet<kClnBufs> cln{bufs};
    // raft_hip_census_*: counts and flag words per read, the flags as bytes, {first bad record, reads with a flag}; staging of the host form --
    // the census's own and not q_*: it lives in the engine library, whose chunk pool backs the columns (kBig), which the side libraries' must not be
    DevBuf cen_cnt{bufs}, cen_flags{bufs}, cen_out{bufs}, cen_ctl{bufs}, cen_len{bufs};
    DevBuf cen_col[6] = {DevBuf{bufs, DevBuf::kBig}, DevBuf{bufs, DevBuf::kBig}, DevBuf{bufs, DevBuf::kBig},
                         DevBuf{bufs, DevBuf::kBig}, DevBuf{bufs, DevBuf::kBig}, DevBuf{bufs, DevBuf::kBig}};
    DevBuf in_col[6] = {DevBuf{bufs, DevBuf::kBig}, DevBuf{bufs, DevBuf::kBig}, DevBuf{bufs, DevBuf::kBig},
                        DevBuf{bufs, DevBuf::kBig}, DevBuf{bufs, DevBuf::kBig}, DevBuf{bufs, DevBuf::kBig}};   // staging for raft_hip_run_host: the columns

    // state of the last pass
    bool ran = false, finished = false;
    int pending_err = RAFT_HIP_OK;
    long long pending_err_index = -1;
    raft_hip_summary sum{};
    FinalizeArgs fa{};                // of the last pass (the cut points are materialised on demand)
    bool cuts_ready = false;
    bool is_lane = false;              // a sub-context of a host pipeline (prepare_lanes)
    void *h_stage = nullptr;           // page-locked staging of a lane: what the host derives from a chunk's columns (window records, offsets)
    size_t h_stage_cap = 0;
    std::vector<DevBuf *> user_bufs;   // raft_hip_device_alloc
    bool emit_cuts = true;             // the pass writes the cut points (final_stars) itself; false: on demand (raft_hip_set_emit_cuts)
    // what the context's last pass over plain columns found out on the way (run_pass: `speculate`): a pass over a stream of the same
    // shape is built on it without the host wait and verifies it on the device
    struct Shape {
        bool valid = false;
        int32_t n_reads = 0, reso = 0, minbins = 0, interval_length = 0, symmetric_mode = 0, tile_q = 0;
        Quantum qz{};                  // the quantum that pass cut its ranges by (run_pass reads its switches at every pass: tile_first is that quantum's)
        int64_t n_rec = 0;
        const void *len = nullptr, *qid = nullptr;
        long long B = 0, RU = 0, CU = 0;
        int n_desc = 0;
        long long desc[kMaxSeg] = {};
        bool had_deep = true;          // its tiles of 2^15 intervals or more (raft_hip_finish): none -> a speculative pass does not launch pileup_deep_kernel
        unsigned long long geom_id = 0;   // which writing of the per-read geometry (cov_off, rep_res_off, tile_first, len_seen) that pass ran on
    } shape;
    // The per-read geometry of a pass depends on the read lengths and the parameters alone.  A speculative pass over the same reads
    // keeps what the context holds (geom_id says that nobody has written the arrays since) and only compares the lengths with the copy
    // the scan left (len_seen): one kernel over 8 bytes per read where the scan's two halves ran over the reads twice.
    unsigned long long geom_id = 0;
    bool speculated = false;           // the pass in flight was built on `shape`
    bool deep_skipped = false;         // ... and without a launch of pileup_deep_kernel (a deep tile then refutes it: kErrDeep)
    bool spec_scanned = false;         // ... and scanned the geometry afresh (raft_hip_finish: kept by later passes if it came through clean)
    unsigned long long spec_geom_id = 0;   // geom_id that scan wrote
    hipStream_t clean_stream = nullptr;
    bool ctrl_clean = false;           // the control block and the hand-out counters were cleared by the last pass's closing kernel, on clean_stream
};


namespace raft {

inline int fail_hip(raft_hip_ctx *c, hipError_t e, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    c->last_error = buf;
    return e == hipErrorOutOfMemory ? RAFT_HIP_ERR_NOMEM : RAFT_HIP_ERR_DEVICE;
}

#define HIP_TRY(c, expr)                                         \
    do {                                                         \
        hipError_t e_ = (expr);                                  \
        if (e_ != hipSuccess) return fail_hip((c), e_, #expr);   \
    } while (0)

inline int check_params(const raft_hip_params *p)
{
    if (!p) return RAFT_HIP_ERR_PARAM;
    if (p->reso <= 0 || p->est_cov <= 0 || p->repeat_length <= 0 || p->interval_length <= 0) return RAFT_HIP_ERR_PARAM;
    if (p->read_length / p->interval_length <= 0) return RAFT_HIP_ERR_PARAM; // div == 0: SIGFPE at chop.hpp:270
    if (p->symmetric_mode < -1 || p->symmetric_mode > 1) return RAFT_HIP_ERR_PARAM;
    return RAFT_HIP_OK;
}

inline void apply_params(raft_hip_ctx *c, const raft_hip_params *p)
{
    c->prm = *p;
    c->high_cov = (int32_t)(p->est_cov * p->cov_mul);            // repeat.hpp:89-90 (int * double, truncated)
    c->div = p->read_length / p->interval_length;                // chop.hpp:248
    c->minbins = (p->repeat_length + p->reso - 1) / p->reso;     // windows a run needs to reach repeat_length
    if (c->minbins < 1) c->minbins = 1;
}

inline int code_from_flags(int flags)
{
    if (flags & (kErrLen | kErrGroup)) return RAFT_HIP_ERR_PARAM;
    if (flags & kErrReadId) return RAFT_HIP_ERR_READ_ID;
    if (flags & kErrCoord) return RAFT_HIP_ERR_COORD;
    if (flags & kErrFragment) return RAFT_HIP_ERR_FRAGMENT;
    if (flags & (kErrInternal | kErrOrder | kErrExtra | kErrHint | kErrDeep)) return RAFT_HIP_ERR_DEVICE;   // (kErrOrder / kErrHint never outlive raft_hip_finish's second run)
    return RAFT_HIP_OK;
}


// ---- what engine.hip provides to the other translation units
void launch_rebase_ids(hipStream_t st, int32_t *ids, long long n, int32_t base);                 // ids[i] -= base (pack.hpp rebase_ids_kernel)
void launch_add_base(hipStream_t st, long long *a, long long n, long long base);                 // a[i] += base (pack.hpp add_base_kernel)
int run_pass(raft_hip_ctx *c, const raft_hip_ctx::PassArgs &in, bool verify_in_kernels);
Ctrl host_ctrl(const raft_hip_ctx *c);             // the control block as the last pass's closing kernel handed it over
int sort_sides(raft_hip_ctx *c, hipStream_t st, long long n_rec, int32_t n_reads, int symmetric, const int32_t *d_qid, const int32_t *d_qs,
               const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te, long long cap_iv, int32_t *o_rid, int32_t *o_s,
               int32_t *o_e, long long *off, int32_t *err_flags, long long *err_index);
int run_grouped(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_len, int64_t n_rec, int32_t n_runs, const int64_t *d_rec_offset,
                const long long *adj, const int32_t *d_qid, const int32_t *d_qs, const int32_t *d_qe, int64_t n_bins,
                const uint32_t *d_win = nullptr);
int pack_coverage(raft_hip_ctx *c, int width);
int sort_exceptions(raft_hip_ctx *c);
int fetch_packed_impl(raft_hip_ctx *c, int32_t width, int64_t *cov_offset, void *cov_packed, int32_t *cov_anchor, int64_t exc_cap, int64_t *exc_index,
                      int32_t *exc_value, int64_t *n_exc, int64_t *rep_offset, int32_t *rep_s, int32_t *rep_e,
                      int64_t *frag_offset, int32_t *frag_read, int32_t *frag_begin, int32_t *frag_end);

// ---- what engine_placement.hip provides: the pileup kernel into K candidate coverage arrays, the fastest kept (called by run_pass's
// pileup phase between ev_pile0 and ev_pile1, with the arguments of the launch it has just made)
int placement_trial(raft_hip_ctx *c, hipStream_t st, const PileupArgs &pa, int ow, bool win, int n_waves, long long N);

} // namespace raft
