#!/usr/bin/env python3
"""Device time of raft_hip_repeat_overlaps_device on the bench-size set (GPU box).

  python tools/repeat_overlaps_time.py [--reads N] [--out profiles/repeat_overlaps_timing.txt]

One process, the set of bench.py's default workload resident in HBM with all six record columns, a finished pass over it on the
context (its repeat annotation is what the call reads: repeats=None).  kernel_seconds of one raft_hip_repeat_overlaps_device call --
HIP events on the context's stream around its launches -- as the median of 10 calls after 2 warm ones, beside the same for
raft_hip_census_device with symmetric = 0 on the same columns in the same process: the yardstick, an existing kernel that streams the
same 24 B per record with the same tallies and candidate gathers.  Also: the digest kernel's share (the call over no records runs the
two kernels over the reads alone), the split of the sides by what their read's digest says, and whether the host form gives the
device form's summary on the same set."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digest_kinds(rep_offset, rep_s, rep_e):
    """Per read what ovl_digest_kernel finds: 0 = no piece, 1 = one piece, 2 = several (the side goes to the CSR arrays)."""
    import numpy as np
    count = np.diff(rep_offset)
    kind = np.minimum(count, 1).astype(np.int8)                    # (one run is one piece: the engine writes no empty run)
    for r in np.flatnonzero(count > 1):
        k0, k1 = int(rep_offset[r]), int(rep_offset[r + 1])
        hi, pieces = int(rep_e[k0]), 1
        for k in range(k0 + 1, k1):
            if int(rep_s[k]) > hi:
                pieces += 1
            hi = max(hi, int(rep_e[k]))
        kind[r] = 1 if pieces == 1 else 2
    return kind


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat_overlaps_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--min-anchor", type=int, default=1000)
    ap.add_argument("--no-host-form", action="store_true", help="skip the host form's run over the same set")
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

    def row(what, secs, n_bytes):
        med = statistics.median(secs)
        say(f"  {what:72s} median {med * 1e3:8.3f} ms  (min {min(secs) * 1e3:.3f}, max {max(secs) * 1e3:.3f}; n = {len(secs)})   "
            f"{n_bytes / 1e9:7.3f} GB moved   {n_bytes / med / 1e12:5.2f} TB/s")
        return med

    eng.run_device(*cols[:4])
    s = eng.finish()
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {s.n_reads} reads, {n_rec} records, {s.n_repeats} repeats; device {torch.cuda.get_device_name(0)}")
    say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; one process; device form, symmetric = 0, "
        f"min_anchor = {args.min_anchor}, the annotation of the context's own pass")
    _, tc = times(lambda: eng.census(*cols, symmetric=False), lambda: eng.last_census_seconds)
    mc = row("yardstick: raft_hip_census_device, symmetric = 0 (census_kernel<true>)", tc, 24 * n_rec + 12 * s.n_reads)
    got, to = times(lambda: eng.repeat_overlaps(*cols, min_anchor=args.min_anchor, symmetric=False), lambda: eng.last_repeat_overlaps_seconds)
    # the six columns and a class byte per record; per read offsets in, the digest out and in again, three words cleared and read
    mo = row("raft_hip_repeat_overlaps_device (ovl_digest_kernel, ovl_class_kernel<true>, ovl_reads_kernel)", to,
             25 * n_rec + (16 + 8 + 8 + 13) * s.n_reads + 8 * s.n_repeats)
    say(f"  repeat_overlaps / census = {mo / mc:.2f}")
    empty = [cols[0]] + [c[:0] for c in cols[1:]]
    _, td = times(lambda: eng.repeat_overlaps(*empty, min_anchor=args.min_anchor, symmetric=False), lambda: eng.last_repeat_overlaps_seconds)
    md = statistics.median(td)
    say(f"  the kernels over the reads alone (no records: ovl_digest_kernel + ovl_reads_kernel) median {md * 1e3:8.3f} ms = {100 * md / mo:.1f} % of the call")
    say("  (outside these events: the class bytes' device-to-device copy into the caller's array, n_rec bytes read and written)")
    fetched = eng.fetch()
    kind = torch.from_numpy(digest_kinds(fetched["rep_offset"], fetched["rep_s"], fetched["rep_e"]).astype(np.int64)).to(dev)
    sides = torch.bincount(kind[cols[1].long()], minlength=3) + torch.bincount(kind[cols[4].long()], minlength=3)
    sides = [int(x) for x in sides.cpu()]
    say(f"sides by their read's digest: none {sides[0]} ({100 * sides[0] / (2 * n_rec):.1f} %), one piece {sides[1]} ({100 * sides[1] / (2 * n_rec):.1f} %), "
        f"sent to the CSR arrays {sides[2]} ({100 * sides[2] / (2 * n_rec):.1f} %)")
    names = ("n_records", "q_touch", "t_touch", "q_repeat", "t_repeat", "both_repeat", "q_contained", "t_contained", "reads_contained",
             "reads_repeat_contained")
    say("device form: " + ", ".join(f"{k} = {got[k]}" for k in names))
    if not args.no_host_form:
        host = eng.repeat_overlaps(*[c.cpu().numpy() for c in cols], min_anchor=args.min_anchor, symmetric=False)
        same = all(host[k] == got[k] for k in names) and np.array_equal(host["read_flags"], got["read_flags"]) and \
            np.array_equal(host["read_touch"], got["read_touch"]) and np.array_equal(host["read_repeat"], got["read_repeat"]) and \
            bool((torch.from_numpy(host["cls"]).to(dev) == got["cls"]).all())
        say(f"the host form over the same set: summary, per-read arrays and class bytes {'identical' if same else 'DIFFER'}")
        assert same
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
