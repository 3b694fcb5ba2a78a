#!/usr/bin/env python3
"""Device time of raft_hip_read_stats and raft_hip_census_device on the bench-size set (GPU box).

  python tools/read_stats_time.py [--reads N] [--out profiles/read_stats_timing.txt]

One process, the set of bench.py's default workload resident in HBM.  Per output width (4, 1, 2): kernel_seconds of
raft_hip_read_stats -- HIP events on the context's stream around its launches -- as the median of 10 calls after 2 warm ones, beside
the same for raft_hip_cov_histogram of the same pass in the same process: the yardstick, which reads the same bytes less the 8 bytes
per read of offsets.  For the census: bytes of the columns read over kernel_seconds, beside a hipMemcpyAsync device-to-device copy of
the same columns timed with events on the same stream."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_stats_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
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
    tid = eng.device_copy(o.tid.contiguous())
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
        say(f"  {what:58s} median {med * 1e3:8.3f} ms  (min {min(secs) * 1e3:.3f}, max {max(secs) * 1e3:.3f}; n = {len(secs)})   "
            f"{n_bytes / 1e9:7.3f} GB read   {n_bytes / med / 1e12:5.2f} TB/s")
        return med

    say("one session on one device: figures of a single run, not a distribution over machines or days")
    results = {}
    for width, name in ((4, "int32_t"), (1, "uint8_t"), (2, "uint16_t")):
        eng.set_output_width(width)
        eng.run_device(*cols)
        s = eng.finish()
        B = s.n_bins
        if width == 4:
            say(f"set: bench.py workload hg002, {s.n_reads} reads, {n_rec} records, {B} windows; device {torch.cuda.get_device_name(0)}")
            say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; one process")
        exc = 0 if width == 4 else eng.packed_device()["exc_index"].numel()
        _, th = times(eng.coverage_histogram, lambda: eng.last_histogram_seconds)
        mh = row(f"yardstick: raft_hip_cov_histogram, width {width} (cov_hist_kernel<{name}>)", th, width * B + 4 * exc)
        st, tr = times(lambda: eng.read_stats(s.high_cov), lambda: eng.last_read_stats_seconds)
        mr = row(f"raft_hip_read_stats, width {width} (read_stats_kernel<{name}>), {exc} listed", tr, width * B + 12 * exc + 8 * s.n_reads)
        say(f"  read_stats / histogram, width {width} = {mr / mh:.2f}")
        assert int(st["cov_sum"].sum()) == s.total_coverage
        results[width] = st
    for w in (1, 2):
        assert all(np.array_equal(results[w][k], results[4][k]) for k in results[4]), f"the width-{w} table differs from the int32 one"
    say("the tables of the three forms agree; sum(cov_sum) = total_coverage")

    c, tc = times(lambda: eng.census(cols[0], cols[1], cols[2], cols[3], tid, symmetric=True), lambda: eng.last_census_seconds)
    census_bytes = 16 * n_rec
    mc = row("raft_hip_census_device, symmetric (16 B per record)", tc, census_bytes)
    assert int(c["intervals"].astype(np.int64).sum()) == n_rec
    dst = [torch.empty_like(t) for t in (cols[1], cols[2], cols[3], tid)]
    ty = []
    for i in range(args.warm + args.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d, t in zip(dst, (cols[1], cols[2], cols[3], tid)):
            d.copy_(t, non_blocking=True)                  # (hipMemcpyAsync, device to device)
        e1.record()
        e1.synchronize()
        if i >= args.warm:
            ty.append(e0.elapsed_time(e1) * 1e-3)
    my = row("yardstick: device-to-device copy of the same four columns", ty, census_bytes)      # (+ as many bytes written)
    say(f"  census / copy = {mc / my:.2f};  {c['n_contained']} of {c['intervals'].size} reads contained")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
