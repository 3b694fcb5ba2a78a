#!/usr/bin/env python3
"""Device time of raft_hip_frag_overlaps_device on the bench-size set (GPU box).

  python tools/fragment_overlaps_time.py [--reads N] [--out profiles/fragment_overlaps_timing.txt]

One process, the set of bench.py's default workload resident in HBM with all six record columns, a finished pass over it on the
context (its fragment rows and its repeat annotation are what the call reads: fragments=None, repeats=None).  kernel_seconds of one
raft_hip_frag_overlaps_device call -- HIP events on the context's stream around its clears and launches -- as the median of 10 calls
after 2 warm ones, beside the same for raft_hip_census_device with symmetric = 0 on the same columns in the same process: the
yardstick, an existing kernel that streams the same 24 B per record.  Also: the share of the kernels that do not look at records (the
call over no records: digests, scan, the kernel over the reads), the split of the sides by the rows of their read, the atomic adds a
side costs on this set, and -- with --host-form -- whether the host form gives the device form's numbers."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fragment_overlaps_timing.txt"))
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
        say(f"  {what:88s} median {med * 1e3:8.3f} ms  (min {min(secs) * 1e3:.3f}, max {max(secs) * 1e3:.3f}; n = {len(secs)})")
        return med

    eng.run_device(*cols[:4])
    s = eng.finish()
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {s.n_reads} reads, {n_rec} records, {s.n_fragments} fragments, {s.n_repeats} repeats; "
        f"device {torch.cuda.get_device_name(0)}")
    say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; one process; device form, symmetric = 0, "
        "the fragment rows and the annotation of the context's own pass")
    _, tc = times(lambda: eng.census(*cols, symmetric=False), lambda: eng.last_census_seconds)
    mc = row("yardstick: raft_hip_census_device, symmetric = 0 (census_kernel<true>)", tc)
    got, tf = times(lambda: eng.fragment_overlaps(*cols, symmetric=False), lambda: eng.last_fragment_overlaps_seconds)
    mf = row("raft_hip_frag_overlaps_device (frag_digest, ovl_digest, frag_side_kernel<true>, scan, frag_reads)", tf)
    say(f"  fragment_overlaps / census = {mf / mc:.2f}")
    empty = [cols[0]] + [c[:0] for c in cols[1:]]
    _, td = times(lambda: eng.fragment_overlaps(*empty, symmetric=False), lambda: eng.last_fragment_overlaps_seconds)
    md = statistics.median(td)
    say(f"  the launches that look at no record (no records: clears, both digests, scan, frag_reads_kernel) median {md * 1e3:8.3f} ms = "
        f"{100 * md / mf:.1f} % of the call")
    say("  (outside these events: the four per-fragment arrays' device-to-device copies into the caller's tensors, 16 B per fragment read and written)")
    fetched = eng.fetch()
    rows = torch.from_numpy(np.diff(fetched["frag_offset"])).to(dev)
    kind = torch.clamp(rows, max=2)
    other = cols[1] != cols[4]
    sides = torch.bincount(kind[cols[1][other].long()], minlength=3) + torch.bincount(kind[cols[4][other].long()], minlength=3)
    sides = [int(x) for x in sides.cpu()]
    total = max(sum(sides), 1)
    say(f"counted sides by the rows of their read: none {sides[0]} ({100 * sides[0] / total:.1f} %), one row, answered from the digest {sides[1]} "
        f"({100 * sides[1] / total:.1f} %), sent to the CSR arrays {sides[2]} ({100 * sides[2] / total:.1f} %); records of a read with itself "
        f"{int((~other).sum())}")
    touch, span, cont = (int(got[k].sum()) for k in ("frag_touch", "frag_span", "frag_contained"))
    say(f"sums over the rows: touching sides {touch}, spanning {span}, containing {cont}; a side that touches adds to two to four slot words, "
        f"one that contains to two more: at least {2 * touch + 2 * cont} 64-bit atomic adds, {(2 * touch + 2 * cont) / max(n_rec, 1):.2f} per record")
    names = ("n_records", "n_fragments", "frags_untouched", "frags_spanned", "frags_contained", "frags_contained_repeat", "reads_whole_spanned",
             "reads_any_contained", "reads_all_contained")
    say("device form: " + ", ".join(f"{k} = {got[k]}" for k in names))
    if args.host_form:
        host = eng.fragment_overlaps(*[c.cpu().numpy() for c in cols], symmetric=False)
        same = all(host[k] == got[k] for k in names) and np.array_equal(host["read_contained"], got["read_contained"]) and \
            all(bool((torch.from_numpy(host[k]).to(dev) == got[k]).all()) for k in ("frag_touch", "frag_span", "frag_contained", "frag_repeat"))
        say(f"the host form over the same set: summary, per-read and per-fragment arrays {'identical' if same else 'DIFFER'}")
        assert same
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
