#!/usr/bin/env python3
"""Device time of raft_hip_cov_histogram on the bench-size set, beside a plain stream of the same array (GPU box).

  python tools/cov_hist_time.py [--reads N] [--out profiles/cov_hist_timing.txt]

One process, the set of bench.py's default workload resident in HBM.  After an int32 pass and after a width-1 pass (and width 2):
kernel_seconds of raft_hip_cov_histogram -- HIP events on the context's stream around its launches -- as the median of 10 calls
after 2 warm ones.  The yardstick is pack_cov_kernel<uint8_t> (raft_amd/csrc/pack.hpp) over the same int32 array: a plain stream of
the same 4 bytes per window, reached through raft_hip_fetch_packed_w's size query after an int32 pass (memset, kernel, an 8-byte
read-back; no array crosses PCIe) and timed with events around the call; it encodes once per pass, so every sample has its own pass."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_hist_timing.txt"))
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
    n_rec = o.n_rec
    del o
    torch.cuda.empty_cache()
    eng.use_torch_stream()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def a_pass(width):
        eng.set_output_width(width)
        eng.run_device(*cols)
        return eng.finish()

    def hist_times():
        t = []
        h = None
        for i in range(args.warm + args.calls):
            h = eng.coverage_histogram()
            if i >= args.warm:
                t.append(eng.last_histogram_seconds)
        return h, t

    def row(what, secs, n_bytes):
        med = statistics.median(secs)
        say(f"  {what:46s} median {med * 1e3:8.3f} ms  (min {min(secs) * 1e3:.3f}, max {max(secs) * 1e3:.3f}; n = {len(secs)})   "
            f"{n_bytes / 1e9:7.3f} GB read   {n_bytes / med / 1e12:5.2f} TB/s")
        return med

    s = a_pass(4)
    B = s.n_bins
    say(f"set: bench.py workload hg002, {n_reads} reads, {n_rec} records, {B} windows; device {torch.cuda.get_device_name(0)}")
    say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; one process")
    h4, t4 = hist_times()
    m4 = row("histogram, int32 cov[] (cov_hist_kernel<int32_t>)", t4, 4 * B)

    none = [C.c_void_p(0)] * 7
    n_exc = C.c_int64(0)
    ty = []
    for i in range(args.warm + args.calls):
        a_pass(4)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng._check(eng._lib.raft_hip_fetch_packed_w(eng._ctx, 1, None, None, 0, None, None, C.byref(n_exc), *none))
        e1.record()
        e1.synchronize()
        if i >= args.warm:
            ty.append(e0.elapsed_time(e1) * 1e-3)
    my = row("yardstick: pack_cov_kernel<uint8_t>, same cov[]", ty, 4 * B)      # (+ 1 B/window written)
    say(f"  histogram / yardstick = {m4 / my:.2f}")

    results = {4: h4}
    for width, name in ((1, "uint8_t"), (2, "uint16_t")):
        s = a_pass(width)
        h, t = hist_times()
        results[width] = h
        exc = eng.packed_device()["exc_index"].numel()
        row(f"histogram, width-{width} codes (cov_hist_kernel<{name}>), {exc} listed", t, width * B + 4 * exc)
    for w in (1, 2):
        assert np.array_equal(results[w], results[4]), f"the width-{w} histogram differs from the int32 one"
    assert int(h4.sum()) == B
    est = engine.estimate_coverage(h4)
    say(f"histograms of the three forms agree; sum = n_bins; {est}  (generator depth {gen_kw['coverage']:g})")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
