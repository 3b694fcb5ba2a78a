#!/usr/bin/env python3
"""Device time of raft_hip_repeat_stats_device on the bench-size set (GPU box).

  python tools/repeat_stats_time.py [--reads N] [--out profiles/repeat_stats_timing.txt]

One process, the set of bench.py's default workload resident in HBM with all six record columns, a finished pass over it on the
context (its repeat annotation and its coverage are what the call reads: repeats=None).  kernel_seconds of one
raft_hip_repeat_stats_device call -- HIP events on the context's stream around its clears and launches -- as the median of 10 calls
after 2 warm ones, with threshold = 0 (the record part: digest, side kernel, runs kernel) and with the coverage part, beside the same
for raft_hip_census_device with symmetric = 0 on the same columns and for raft_hip_read_stats in the same process: the yardsticks,
existing kernels that stream the same 24 B per record and the same coverage array.  Also: the launches that look at no record, the
split of the sides by the runs of their read, the atomic adds the record part sends on this set, the windows the coverage part reads
against the pass's, and -- with --host-form -- whether the host form gives the device form's numbers."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat_stats_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--host-form", action="store_true", help="also run the host form over the same set and compare")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import DEFAULT_READS, WORKLOADS
    from raft_amd import engine
    from raft_amd.params import RaftParams
    from raft_amd.synth import make_overlaps

    gen_kw, est_cov, _ = WORKLOADS["hg002"]
    n_reads = args.reads or DEFAULT_READS["hg002"]
    dev = "cuda:0"
    p = RaftParams(est_cov=est_cov, symmetric_mode=1)
    eng = engine.Engine(p, device=0)
    o = make_overlaps(n_reads, seed=20241008, device=dev, **gen_kw)
    cols = [eng.device_copy(t.contiguous()) for t in (o.read_len,) + tuple(o.columns())]      # (the engine's placement, as in bench.py)
    n_rec = o.n_rec
    del o
    torch.cuda.empty_cache()
    eng.use_torch_stream()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def times(call, seconds):
        t, out = [], None
        for i in range(args.warm + args.calls):
            out = call()
            if i >= args.warm:
                t.append(seconds())
        return out, t

    def row(what, secs):
        med = statistics.median(secs)
        say(f"  {what:96s} median {med * 1e3:8.3f} ms  (min {min(secs) * 1e3:.3f}, max {max(secs) * 1e3:.3f}; n = {len(secs)})")
        return med

    eng.run_device(*cols[:4])
    s = eng.finish()
    thr = p.high_cov
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {s.n_reads} reads, {n_rec} records, {s.n_bins} windows, {s.n_repeats} repeats; "
        f"device {torch.cuda.get_device_name(0)}")
    say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; one process; device form, symmetric = 0, "
        f"the annotation and the int32 coverage of the context's own pass, threshold {thr}")
    _, tc = times(lambda: eng.census(*cols, symmetric=False), lambda: eng.last_census_seconds)
    mc = row("yardstick: raft_hip_census_device, symmetric = 0 (census_kernel<true>)", tc)
    _, tr = times(lambda: eng.read_stats(thr), lambda: eng.last_read_stats_seconds)
    mr = row("yardstick: raft_hip_read_stats (read_stats_kernel<int32_t>)", tr)
    got0, t0 = times(lambda: eng.repeat_stats(*cols, symmetric=False, threshold=0), lambda: eng.last_repeat_stats_seconds)
    m0 = row("raft_hip_repeat_stats_device, threshold = 0 (rst_digest, rst_side_kernel<true>, rst_runs)", t0)
    got, t1 = times(lambda: eng.repeat_stats(*cols, symmetric=False, threshold=thr), lambda: eng.last_repeat_stats_seconds)
    m1 = row("raft_hip_repeat_stats_device with the coverage part (+ rst_cov_kernel)", t1)
    say(f"  record part / census = {m0 / mc:.2f}; coverage part = {(m1 - m0) * 1e3:.3f} ms, coverage part / read_stats = {(m1 - m0) / mr:.2f}")
    _, td = times(lambda: eng.repeat_stats(cols[0], symmetric=False, threshold=0), lambda: eng.last_repeat_stats_seconds)
    md = statistics.median(td)
    say(f"  the launches that look at no record (no records: clears, rst_digest_kernel, rst_runs_kernel) median {md * 1e3:8.3f} ms = "
        f"{100 * md / m0:.1f} % of the record part")
    fetched = eng.fetch(coverage=False)
    rep_off, rep_s, rep_e = fetched["rep_offset"], fetched["rep_s"].astype(np.int64), fetched["rep_e"].astype(np.int64)
    real = np.add.reduceat(np.r_[(rep_e > rep_s).astype(np.int64), 0], rep_off[:-1]) * (np.diff(rep_off) > 0)
    kind = torch.from_numpy(np.minimum(real, 2)).to(dev)
    other = cols[1] != cols[4]
    sides = torch.bincount(kind[cols[1].long()], minlength=3) + torch.bincount(kind[cols[4][other].long()], minlength=3)
    sides = [int(x) for x in sides.cpu()]
    total = max(sum(sides), 1)
    say(f"counted sides by the non-empty runs of their read: none {sides[0]} ({100 * sides[0] / total:.1f} %: one 16-byte gather), one run, joined "
        f"before they are added {sides[1]} ({100 * sides[1] / total:.1f} %), several runs, walked {sides[2]} ({100 * sides[2] / total:.1f} %); "
        f"reads with none / one / several: {int((real == 0).sum())} / {int((real == 1).sum())} / {int((real > 1).sum())}")
    say(f"sums over the runs: touching sides {got['sides_touch']}, spanning {got['sides_span']}, inside {got['sides_inside']}: a walked side sends "
        f"one 64-bit atomic add per run it touches and one more when it lies inside; joined sides send one pair per slot and wave")
    say(f"coverage part: {got['windows']} windows read of the pass's {s.n_bins} ({100 * got['windows'] / max(s.n_bins, 1):.1f} %), a wave per run, "
        f"{got['windows'] / max(got['n_runs'], 1):.0f} windows a run")
    say("device form: " + ", ".join(f"{k} = {got[k]}" for k, _ in engine._RstSummary._fields_))
    assert all(np.array_equal(got[k], got0[k]) for k in ("run_touch", "run_span", "run_inside", "run_flags"))
    if args.host_form:
        host = eng.repeat_stats(*[c.cpu().numpy() for c in cols], symmetric=False, threshold=thr)
        same = all(host[k] == got[k] for k, _ in engine._RstSummary._fields_) and \
            all(np.array_equal(host[k], got[k]) for k in eng.RUN_COUNTS + eng.RUN_COVERAGE + ("run_flags",))
        say(f"the host form over the same set: summary and per-run arrays {'identical' if same else 'DIFFER'}")
        assert same
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
