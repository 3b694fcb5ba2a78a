#!/usr/bin/env python3
"""Device time of raft_hip_containment_device on the bench's set against raft_hip_overlap_ends_device over the same stream in the same
process, and against the same rule walked sequentially on one host core (GPU box).

  python tools/containment_probe.py [--reads N] [--out profiles/containment_timing.txt]

Steps, each a process of its own under its own time limit; a step that fails or runs out of time ends the probe, and nothing more is
started on the device.  Step "device": the set resident in HBM; kernel_seconds of the whole call -- HIP events on the context's stream
around its launches -- as the median of ``--calls`` calls after ``--warm`` warm ones; beside it raft_hip_overlap_ends_device, which
streams the same 25 B per record once.  The step leaves the arrays in a file for step "walk": tools/containment_walk (built here with
g++ -O2 if it is not there), one host thread; its counts and its checksum over root, root_pos, depth and the strand must equal the
device's.  The kernels one by one are a kernel trace's business, in a run of its own: --trace runs the device step alone, two calls,
for a profiler to wrap."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WALK = os.path.join(ROOT, "tools", "containment_walk")
H, F = 1000, 800


def child(args):
    import numpy as np
    import torch

    from bench import DEFAULT_READS, WORKLOADS
    from raft_amd import engine
    from raft_amd.params import RaftParams
    from raft_amd.synth import make_overlaps

    dev = "cuda:0"
    gen_kw, est_cov, _ = WORKLOADS["hg002"]
    eng = engine.Engine(RaftParams(est_cov=est_cov), device=0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    n_reads = args.reads or DEFAULT_READS["hg002"]
    o = make_overlaps(n_reads, seed=20241008, device=dev, **gen_kw)
    tensors = [t.contiguous() for t in (o.read_len,) + tuple(o.columns())]
    strand = (torch.rand(o.n_rec, device=dev, generator=gen) < 0.5).to(torch.uint8)
    del o
    cols = [eng.device_copy(t) for t in tensors]                        # (the engine's placement, as in bench.py)
    strand = eng.device_copy(strand)
    n_rec = int(cols[1].numel())
    del tensors
    torch.cuda.empty_cache()
    eng.use_torch_stream()

    def times(fn):
        t = []
        for i in range(args.warm + args.calls):
            v = fn()
            if i >= args.warm:
                t.append(v)
        return t
    last = {}

    def forest():
        last["r"] = eng.containment(*cols, strand, max_overhang=H, min_ratio_permille=F, symmetric=True)
        return last["r"]["kernel_seconds"]

    def ends_time():
        eng.overlap_ends(*cols, strand, max_overhang=H, min_ratio_permille=F, symmetric=True)
        return eng.last_overlap_ends_seconds
    out = {"n_reads": n_reads, "n_rec": n_rec, "device": torch.cuda.get_device_name(0), "forest": times(forest), "ends": times(ends_time)}
    r = last["r"]
    weights = (np.arange(n_reads, dtype=np.int64) & 1023) + 1
    value = r["root"].astype(np.int64) + r["root_pos"] + r["depth"] + (r["flags"] & engine.CTN_ROOT_REV != 0)
    out["summary"] = dict(r["summary"], checksum=int((value * weights).sum()))
    if args.dump:
        with open(args.dump, "wb") as f:
            np.array([n_reads, n_rec, H, F, 1], np.int64).tofile(f)
            for t in cols + [strand]:
                t.cpu().numpy().tofile(f)
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="reads of the bench's set; 0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "containment_timing.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--walks", type=int, default=1, help="repeats of the host walk")
    ap.add_argument("--step-limit", type=int, default=300, help="seconds one step may take")
    ap.add_argument("--trace", action="store_true", help="the device step alone, in this process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dump", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or args.trace:
        if args.trace:
            args.calls, args.warm = 2, 1
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if not os.path.exists(WALK):
        subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "containment_walk.cpp"), "-o", WALK], check=True)
    ms = lambda v: f"median {statistics.median(v) * 1e3:9.3f} ms  (min {min(v) * 1e3:.3f}, max {max(v) * 1e3:.3f}; n = {len(v)})"
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream around the call's launches; device form, "
        f"max_overhang = {H}, min_ratio = {F}, symmetric = 1")
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "bench.bin")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reads", str(args.reads), "--calls", str(args.calls), "--warm", str(args.warm),
               "--dump", dump]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
        except subprocess.TimeoutExpired:
            say(f"step device: not through after {args.step_limit} s; the probe ends here")
            return 1
        found = [ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")]
        if r.returncode != 0 or len(found) != 1:
            say(f"step device: exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}")
            return 1
        d = json.loads(found[0][7:])
        print("device step done", flush=True)
        try:
            w = subprocess.run([WALK, dump, str(args.walks)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
        except subprocess.TimeoutExpired:
            say(f"step walk: not through after {args.step_limit} s; the probe ends here")
            return 1
    walk = [ln for ln in w.stdout.split("\n") if ln.startswith("WALK ")]
    if w.returncode != 0 or len(walk) != 1:
        say(f"step walk: exit status {w.returncode}; the probe ends here\n{w.stdout[-2000:]}")
        return 1
    f = walk[0].split()
    counts, host_s = [int(x) for x in f[1:7]], [float(x) for x in f[7:]]
    s = d["summary"]
    say(f"set: bench.py workload hg002, strand drawn at random; {d['n_reads']} reads, {d['n_rec']} records; device {d['device']}")
    say(f"  raft_hip_containment_device  {ms(d['forest'])}  launches = {s['launches']}")
    say(f"    containment views = {s['containment_views']} ({1000 * s['containment_views'] // max(d['n_rec'], 1)} per mille of the records), not longer = "
        f"{s['views_not_longer']}, reads with a parent = {s['reads_with_parent']}, orphans = {s['orphans']}, roots with a tree = {s['roots_with_tree']}, "
        f"deepest = {s['greatest_depth']}, largest tree = {s['largest_tree_reads']} reads, checksum = {s['checksum']}")
    say(f"  yardstick: raft_hip_overlap_ends_device, same stream, same H and F  {ms(d['ends'])};  containment / overlap_ends = "
        f"{statistics.median(d['forest']) / statistics.median(d['ends']):.2f}")
    say(f"  host walk (tools/containment_walk, one thread, -O2)  median {statistics.median(host_s):8.3f} s  (n = {len(host_s)})  walk / device call = "
        f"{statistics.median(host_s) / statistics.median(d['forest']):.0f}")
    ok = counts == [d["n_rec"], s["containment_views"], s["views_not_longer"], s["reads_with_parent"], s["greatest_depth"], s["checksum"]]
    say(f"  the walk's counts and checksum equal the device's: {'yes' if ok else 'NO ' + str(counts)}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
