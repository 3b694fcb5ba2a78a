// engine_placement.hip -- where buffers lie: the per-device pool of physical chunks (trim, what it holds), the placement policy, the
// placement trial and its report, device memory for the callers' input columns, page-locking of caller memory.  The buffers themselves
// (DevBuf: virtual ranges over pooled chunks) are in engine_ctx.hpp; DESIGN.md I.4 says why any of this exists.
#include "engine_ctx.hpp"

namespace raft {

// ---- where the coverage array lies, decided by measurement: OPT-IN (raft_hip_set_placement_trial / RAFT_PLACEMENT_TRIALS=<k>;
// round 5 ran it by default, round 6 does not: the driver's own A/B showed 0.2 % between the policies, and a one-shot caller
// paid 2 K - 1 extra launches and K - 1 coverage-sized allocations for nothing).  What this kernel gets from the part follows
// the array it stores into, and not by the KIND of memory: two hipMalloc blocks of one process gave 2.24 and 2.63 ms, two chunk
// mappings 2.49 and 2.67.  A context that asked for a trial draws K - 1 more arrays at the first pass that makes
// a coverage array of a GiB or more -- plain blocks and chunk mappings in turn, each only while the device keeps its reserve
// free behind it --, runs the kernel into each of them warm, and keeps the one it was fastest with.
// Called by run_pass right behind the pass's own launch of the pileup kernel, with that launch's arguments.
int placement_trial(raft_hip_ctx *c, hipStream_t st, const PileupArgs &pa, int ow, bool win, int n_waves, long long N)
{
    const int kTrials = c->trial_candidates;
    Ctrl *ctrl = c->ctrl.as<Ctrl>();
    c->cov_trial_cap = c->cov.cap;
    struct TrialGuard {                       // every way out of this function releases the candidates and the events
        std::vector<DevBuf> cand;
        std::vector<hipEvent_t> ev;
        ~TrialGuard()
        {
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
            for (DevBuf &b : cand) b.release();
        }
    } tg;
    tg.cand.resize((size_t)kTrials - 1);
    tg.ev.assign((size_t)2 * kTrials, nullptr);
    std::vector<DevBuf> &cand = tg.cand;
    std::vector<hipEvent_t> &ev = tg.ev;
    int n_cand = 0;
    for (int k = 0; k + 1 < kTrials; ++k) {
        // a candidate is drawn only while an eighth of the device's memory (8 GiB at least) stays free behind it: the same
        // reserve map_chunks keeps for its spare chunks (torch, RCCL and other processes live there)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); break; }
        if (free_b < c->cov.cap + std::max<size_t>(size_t(8) << 30, total_b / 8)) break;
        cand[(size_t)k].big = (k & 1) != 0;       // plain block, chunk mapping, plain block, ...
        if (cand[(size_t)k].ensure(c->cov.cap) != hipSuccess) { (void)hipGetLastError(); break; }
        ++n_cand;
    }
    bool ok = n_cand > 0;
    for (size_t i = 0; ok && i < ev.size(); ++i) ok = hipEventCreate(&ev[i]) == hipSuccess;
    if (!ok) return RAFT_HIP_OK;
    // (the pass's own launch was the context's first -- code going to the device, cold translations: 3 ms, or 200 -- and says
    // nothing; the first run into an array pays for its first touch; the second is the measurement.  What a run leaves
    // behind and the next must not see: the reads' repeat counters, the hand-out counters)
    auto one_run = [&](int32_t *cov_p, hipEvent_t e0, hipEvent_t e1) -> int {
        PileupArgs x = pa;
        x.cov = cov_p;
        x.tile_batch = (pa.tile_batch & ~kCovLineBit) | cov_line_bit(cov_p);
        HIP_TRY(c, hipMemsetAsync(c->rep_cnt.p, 0, (size_t)std::max(N, 1LL) * 4, st));
        HIP_TRY(c, hipMemsetAsync(c->wave_ctr.p, 0, (size_t)kWaveCounters * kCtrStride * 4, st));
        HIP_TRY(c, hipMemsetAsync(&ctrl->n_deep, 0, 4, st));
        if (e0) HIP_TRY(c, hipEventRecord(e0, st));
        launch_wave_variant(ow, win, st, x.n_seg, c->tile_cuts.p, &x, n_waves);
        if (e1) HIP_TRY(c, hipEventRecord(e1, st));
        return RAFT_HIP_OK;
    };
    int trc = RAFT_HIP_OK;
    for (int k = 0; k < n_cand && trc == RAFT_HIP_OK; ++k) trc = one_run(cand[(size_t)k].as<int32_t>(), nullptr, nullptr);
    if (trc == RAFT_HIP_OK) trc = one_run(c->cov.as<int32_t>(), ev[0], ev[1]);
    for (int k = 0; k < n_cand && trc == RAFT_HIP_OK; ++k) trc = one_run(cand[(size_t)k].as<int32_t>(), ev[(size_t)2 * k + 2], ev[(size_t)2 * k + 3]);
    if (trc != RAFT_HIP_OK) { (void)hipStreamSynchronize(st); return trc; }      // (nothing in flight may still use a candidate)
    HIP_TRY(c, hipEventSynchronize(ev[(size_t)2 * n_cand + 1]));
    float best = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&best, ev[0], ev[1]));
    c->trial_ms[0] = best; c->trial_ms[1] = 0.0;
    int keep = -1;
    for (int k = 0; k < n_cand; ++k) {
        float t = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&t, ev[(size_t)2 * k + 2], ev[(size_t)2 * k + 3]));
        if (c->trial_ms[1] == 0.0 || t < c->trial_ms[1]) c->trial_ms[1] = t;
        if (t < best * 0.985f) { best = t; keep = k; }      // (a candidate has to win by more than the noise of two launches)
    }
    c->trial_kept = keep >= 0 ? (cand[(size_t)keep].big ? 2 : 1) : 0;
    if (keep >= 0) { std::swap(c->cov, cand[(size_t)keep]); c->cov_trial_cap = c->cov.cap; }
    // (whichever array is kept holds this pass's coverage: every run wrote all of it)
    return RAFT_HIP_OK;
}

} // namespace raft

extern "C" {

int64_t raft_hip_trim(int device_id, int64_t keep_bytes)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev || keep_bytes < 0) return -(int64_t)RAFT_HIP_ERR_PARAM;
    // (hipMemRelease needs no current device: the caller's stays as it is)
    return (int64_t)ChunkPool::of(device_id).trim((size_t)(keep_bytes / (int64_t)DevBuf::kChunk)) * (int64_t)DevBuf::kChunk;
}

int32_t raft_hip_set_placement(int32_t spread)
{
    DevBuf::policy_explicit().store(true);
    return (int32_t)DevBuf::policy().exchange(spread < 0 ? 0 : std::min(spread, 64));
}

int raft_hip_placement_trial(raft_hip_ctx *c, double *first_ms, double *best_other_ms, int32_t *kept)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (first_ms) *first_ms = c->trial_ms[0];
    if (best_other_ms) *best_other_ms = c->trial_ms[1];
    if (kept) *kept = c->trial_kept;
    return c->trial_ms[0] > 0.0 ? RAFT_HIP_OK : RAFT_HIP_ERR_STATE;
}

int raft_hip_set_placement_trial(raft_hip_ctx *c, int32_t candidates)
{
    if (!c || candidates < 0 || candidates > 8) return RAFT_HIP_ERR_PARAM;
    c->trial_candidates = candidates;
    return RAFT_HIP_OK;
}

int64_t raft_hip_pool_bytes(int device_id)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev || device_id >= 64) return -(int64_t)RAFT_HIP_ERR_PARAM;
    ChunkPool &pool = ChunkPool::of(device_id);
    std::lock_guard<std::mutex> lk(pool.mu);
    return (int64_t)pool.free_chunks.size() * (int64_t)DevBuf::kChunk;
}

int raft_hip_device_alloc(raft_hip_ctx *c, int64_t bytes, void **dptr)
{
    if (!c || !dptr || bytes < 0) return RAFT_HIP_ERR_PARAM;
    *dptr = nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return RAFT_HIP_ERR_DEVICE;
    DevBuf *b = new (std::nothrow) DevBuf();
    if (!b) return RAFT_HIP_ERR_NOMEM;
    b->big = true;
    if (b->ensure((size_t)std::max<int64_t>(bytes, 1)) != hipSuccess) { (void)hipGetLastError(); delete b; return RAFT_HIP_ERR_NOMEM; }
    c->user_bufs.push_back(b);
    *dptr = b->p;
    return RAFT_HIP_OK;
}

int raft_hip_device_free(raft_hip_ctx *c, void *dptr)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (!dptr) return RAFT_HIP_OK;
    for (size_t i = 0; i < c->user_bufs.size(); ++i)
        if (c->user_bufs[i]->p == dptr) {
            (void)hipSetDevice(c->device);
            c->user_bufs[i]->release();
            delete c->user_bufs[i];
            c->user_bufs.erase(c->user_bufs.begin() + (long)i);
            return RAFT_HIP_OK;
        }
    return RAFT_HIP_ERR_PARAM;
}

// Page-locking of caller memory.  The host pipelines move gigabytes each way; from pageable memory the runtime stages them
// through its own bounce buffers.  Measured on the MI355X box (tools/pin_rate.py): hipHostRegister pins pages that have been
// touched at ~120 GB/s (16 ms for 2 GB) and untouched ones at ~20 GB/s (their first touch), after which copies run at the
// link's 53 GB/s.
int raft_hip_host_register(void *ptr, uint64_t bytes)
{
    if (!ptr || bytes == 0) return RAFT_HIP_ERR_PARAM;
    const hipError_t e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterPortable);
    if (e == hipSuccess) return RAFT_HIP_OK;
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? RAFT_HIP_ERR_NOMEM : RAFT_HIP_ERR_DEVICE;
}

int raft_hip_host_unregister(void *ptr)
{
    if (!ptr) return RAFT_HIP_ERR_PARAM;
    if (hipHostUnregister(ptr) == hipSuccess) return RAFT_HIP_OK;
    (void)hipGetLastError();
    return RAFT_HIP_ERR_DEVICE;
}


} // extern "C"
