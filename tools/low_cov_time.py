#!/usr/bin/env python3
"""Device time of raft_hip_low_coverage on the bench-size set (GPU box).

  python tools/low_cov_time.py [--reads N] [--out profiles/low_cov_timing.txt]

One process, the set of bench.py's default workload resident in HBM.  Per output width (4, 2, 1): kernel_seconds of one
raft_hip_low_coverage call at low_cov = 0 -- HIP events on the context's stream around its launches, both halves of the call -- as the
median of 10 calls after 2 warm ones, beside the same for raft_hip_cov_histogram of the same pass in the same process: the yardstick,
which reads the same array once.  By the byte count the call should cost the histogram plus the bitmap passes: 1 + 3/32 of its bytes."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "low_cov_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--low-cov", type=int, default=0)
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
    cols = [eng.device_copy(t.contiguous()) for t in (o.read_len, o.qid, o.qs, o.qe)]      # (the engine's placement, as in bench.py)
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

    def row(what, secs, n_bytes):
        med = statistics.median(secs)
        say(f"  {what:66s} median {med * 1e3:8.3f} ms  (min {min(secs) * 1e3:.3f}, max {max(secs) * 1e3:.3f}; n = {len(secs)})   "
            f"{n_bytes / 1e9:7.3f} GB read   {n_bytes / med / 1e12:5.2f} TB/s")
        return med

    say("one session on one device: figures of a single run, not a distribution over machines or days")
    results = {}
    for width, name in ((4, "int32_t"), (2, "uint16_t"), (1, "uint8_t")):
        eng.set_output_width(width)
        eng.run_device(*cols)
        s = eng.finish()
        B = s.n_bins
        if width == 4:
            say(f"set: bench.py workload hg002, {s.n_reads} reads, {n_rec} records, {B} windows; device {torch.cuda.get_device_name(0)}")
            say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; one process; low_cov = {args.low_cov}")
        _, th = times(eng.coverage_histogram, lambda: eng.last_histogram_seconds)
        mh = row(f"yardstick: raft_hip_cov_histogram, width {width} (cov_hist_kernel<{name}>)", th, width * B)
        got, tl = times(lambda: eng.low_coverage(args.low_cov), lambda: eng.last_low_coverage_seconds)
        # cov[] once, the bitmap written once and read by count and fill (with the read-start bitmap), offsets and lengths per read
        ml = row(f"raft_hip_low_coverage, width {width} (low_mark_kernel<{name}> ...), {got['n_runs']} runs", tl,
                 width * B + 5 * B // 8 + 28 * s.n_reads + 24 * got["n_runs"])
        say(f"  low_coverage / histogram, width {width} = {ml / mh:.2f}")
        results[width] = got
    for w in (1, 2):
        assert all(np.array_equal(results[w][k], results[4][k]) for k in results[4]), f"the width-{w} answer differs from the int32 one"
    g = results[4]
    say(f"the answers of the three forms agree: {g['n_runs']} runs, {g['total_low_windows']} low windows, {g['reads_with_runs']} reads with a run, "
        f"{g['reads_interior']} with an interior run, {g['reads_uncovered']} uncovered")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
