// pipeline_plan_print.cpp -- what the planner of the chunked host pipeline (raft_amd/csrc/pipeline_plan.hpp) makes of ONE input, as text:
// the sorted runs it believes in (guess_segments, or the runs of grouped offsets as engine_pipeline.hip choose_route takes them), the
// chunk plan (plan_chunks, no ramp) and every context's place for 1, 2 and 3 contexts (place_jobs).  tests/test_pipeline_cases.py holds
// the output against the plain-Python model and the literal claims of tests/pipeline_cases.py.  No device, no HIP.
//
// stdin:  reso minbins interval_length want d4 | n_reads len... | form n_runs n_rec | form 0: qid[n_rec]; form 1: off[n_runs * (n_reads + 1)]
// stdout: "runs n s0 .. sn" (n = -1: no handful of runs), "chunk r0 r1 win_lo n_rec(run 0) ..", "jobs n_ctx n_job bins rep frag" and
//         per job "job first_chunk n_chunks bins0 rep_room frag_room"
#include "../raft_amd/csrc/pipeline_plan.hpp"

#include <cstdio>
#include <iostream>

using namespace raft;

int main()
{
    long long reso, minbins, interval_length, want, d4, n_reads, form, n_runs, n_rec;
    if (!(std::cin >> reso >> minbins >> interval_length >> want >> d4 >> n_reads)) return 2;
    std::vector<int32_t> len((size_t)n_reads), qid;
    for (auto &x : len) std::cin >> x;
    std::cin >> form >> n_runs >> n_rec;
    std::vector<int64_t> off;
    HostInput in;
    in.n_reads = (int32_t)n_reads; in.read_len = len.data(); in.n_rec = n_rec;
    long long seg[kPlanSeg + 1] = {};
    int n_seg = -1;
    if (form == 0) {
        qid.resize((size_t)n_rec);
        for (auto &x : qid) std::cin >> x;
        in.qid = qid.data();
        n_seg = guess_segments(qid.data(), n_rec, seg);
    } else {
        off.resize((size_t)(n_runs * (n_reads + 1)));
        for (auto &x : off) std::cin >> x;
        in.n_runs = (int32_t)n_runs; in.rec_offset = off.data();
        if (n_runs <= kPlanSeg) {
            n_seg = (int)n_runs;
            for (int g = 0; g < n_runs; ++g) seg[g] = in.off_at(g, 0);
            seg[n_runs] = n_rec;
        }
    }
    if (!std::cin) return 2;
    printf("runs %d", n_seg);
    for (int g = 0; g <= n_seg; ++g) printf(" %lld", seg[g]);
    printf("\n");
    if (n_seg < 1) return 0;
    const std::vector<ChunkPlan> plan = plan_chunks(in, seg, n_seg, (int)std::min(want, n_reads), false, d4 != 0, (int32_t)reso);
    for (const ChunkPlan &cp : plan) {
        printf("chunk %d %d %lld", cp.r0, cp.r1, cp.win_lo);
        long long sum = 0;
        for (int g = 0; g < n_seg; ++g) { printf(" %lld", cp.piece[g].hi - cp.piece[g].lo); sum += cp.piece[g].hi - cp.piece[g].lo; }
        printf("\n");
        if (sum != cp.n_rec) return 3;
    }
    for (int n_ctx = 1; n_ctx <= 3 && !plan.empty(); ++n_ctx) {
        const int n_job = std::min<int>(n_ctx, (int)plan.size());
        PlaceCaps caps;
        const std::vector<JobPlace> at = place_jobs(plan, n_job, len.data(), minbins, interval_length, WindowDiv((int32_t)reso), &caps);
        printf("jobs %d %d %lld %lld %lld\n", n_ctx, n_job, caps.bins, caps.rep, caps.frag);
        for (const JobPlace &J : at) printf("job %d %d %lld %lld %lld\n", J.first_chunk, J.n_chunks, J.bins0, J.rep_room, J.frag_room);
    }
    return 0;
}
