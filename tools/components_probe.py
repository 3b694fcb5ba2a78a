#!/usr/bin/env python3
"""Device time of raft_hip_components_device on the bench's set against the same rule with a sequential union-find on one host core
(GPU box).

  python tools/components_probe.py [--reads N] [--other-lib PATH --other-name TEXT] [--out profiles/components_timing.txt]

Steps, each a process of its own under its own time limit; a step that fails or runs out of time ends the probe, and nothing more is
started on the device.  Step "device": the set of bench.py's default workload resident in HBM with its six record columns and a
strand column drawn at random; kernel_seconds of the whole call -- HIP events on the context's stream around its seven launches -- for
the masks PROPER and ALL, each as the median of 10 calls after 2 warm ones; the same call without records (every launch but the link
kernel, over a forest of roots); beside them, in the same process, raft_hip_overlap_ends_device, which streams the same 25 B per
record.  With --other-lib the step runs once more on a second build of libraft_hip_cc.so (the other setting of RAFT_CC_HALVE).  The
first step leaves the arrays in a file for step "walk": tools/components_walk (built here with g++ -O2 if it is not there), one host
thread, 3 repeats under PROPER; its counts and its checksum over component[] must equal the device's.  The link kernel alone is a
kernel trace's business, in a run of its own: --trace runs the device step alone, three calls per mask, for a profiler to wrap."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WALK = os.path.join(ROOT, "tools", "components_walk")
H, F = 1000, 800


def child(args):
    import numpy as np
    import torch

    from bench import DEFAULT_READS, WORKLOADS
    from raft_amd import engine
    from raft_amd.params import RaftParams
    from raft_amd.synth import make_overlaps

    if args.cc_lib:
        engine._SIDE_LATER["cc"] = (os.path.abspath(args.cc_lib),) + engine._SIDE_LATER["cc"][1:]
    gen_kw, est_cov, _ = WORKLOADS["hg002"]
    n_reads = args.reads or DEFAULT_READS["hg002"]
    dev = "cuda:0"
    eng = engine.Engine(RaftParams(est_cov=est_cov), device=0)
    o = make_overlaps(n_reads, seed=20241008, device=dev, **gen_kw)
    cols = [eng.device_copy(t.contiguous()) for t in (o.read_len,) + tuple(o.columns())]      # (the engine's placement, as in bench.py)
    n_rec = o.n_rec
    del o
    torch.cuda.empty_cache()
    eng.use_torch_stream()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    strand = eng.device_copy((torch.rand(n_rec, device=dev, generator=gen) < 0.5).to(torch.uint8))
    qid = cols[1]
    sorted_queries = bool((qid[1:] >= qid[:-1]).all()) if n_rec > 1 else True

    def times(fn):
        t = []
        for i in range(args.warm + args.calls):
            v = fn()
            if i >= args.warm:
                t.append(v)
        return t

    res = {}

    def cc(mask, records=True):
        given = cols if records else [cols[0]] + [c[:0] for c in cols[1:]]
        r = eng.components(*given, strand if records else strand[:0], H, F, mask, True)
        res[mask if records else 0] = r
        return r["kernel_seconds"]
    out = {"n_reads": n_reads, "n_rec": n_rec, "sorted_queries": sorted_queries, "device": torch.cuda.get_device_name(0)}
    for name, mask in (("proper", engine.CC_KINDS_PROPER), ("all", engine.CC_KINDS_ALL)):
        out[name] = times(lambda: cc(mask))
        r = res[mask]
        weights = (np.arange(n_reads, dtype=np.int64) & 1023) + 1
        out[name + "_summary"] = dict(r["summary"], checksum=int((r["component"].astype(np.int64) * weights).sum()), launches=r["launches"])
    out["no_records"] = times(lambda: cc(engine.CC_KINDS_PROPER, records=False))

    def ends():
        eng.overlap_ends(*cols, strand, max_overhang=H, min_ratio_permille=F, symmetric=True)
        return eng.last_overlap_ends_seconds
    out["ends"] = times(ends)
    if args.dump:
        with open(args.dump, "wb") as f:
            np.array([n_reads, n_rec, H, F, engine.CC_KINDS_PROPER, 1], np.int64).tofile(f)
            for t in cols + [strand]:
                t.cpu().numpy().tofile(f)
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--name", default="path halving on (RAFT_CC_HALVE=1, the build's default)", help="what the library of the build is")
    ap.add_argument("--other-lib", default="", help="a second libraft_hip_cc.so, timed as well")
    ap.add_argument("--other-name", default="path halving off (RAFT_CC_HALVE=0)")
    ap.add_argument("--step-limit", type=int, default=300, help="seconds one step may take")
    ap.add_argument("--trace", action="store_true", help="the device step alone, in this process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cc-lib", default="", help=argparse.SUPPRESS)
    ap.add_argument("--dump", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or args.trace:
        if args.trace:
            args.calls, args.warm = 3, 1
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if not os.path.exists(WALK):
        subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "components_walk.cpp"), "-o", WALK], check=True)
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "set.bin")
        runs = []
        for name, lib in [(args.name, "")] + ([(args.other_name, args.other_lib)] if args.other_lib else []):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reads", str(args.reads), "--calls", str(args.calls), "--warm", str(args.warm)]
            cmd += ["--cc-lib", lib] if lib else ["--dump", dump]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
            except subprocess.TimeoutExpired:
                say(f"step device ({name}): not through after {args.step_limit} s; the probe ends here")
                return 1
            found = [ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")]
            if r.returncode != 0 or len(found) != 1:
                say(f"step device ({name}): exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}")
                return 1
            runs.append((name, json.loads(found[0][7:])))
            print(f"device step done: {name}", flush=True)
        try:
            w = subprocess.run([WALK, dump, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
        except subprocess.TimeoutExpired:
            say(f"step walk: not through after {args.step_limit} s; the probe ends here")
            return 1
    walk = [ln for ln in w.stdout.split("\n") if ln.startswith("WALK ")]
    if w.returncode != 0 or len(walk) != 1:
        say(f"step walk: exit status {w.returncode}; the probe ends here\n{w.stdout[-2000:]}")
        return 1
    f = walk[0].split()
    counts, host_s = [int(x) for x in f[1:6]], [float(x) for x in f[6:]]
    d = runs[0][1]
    ms = lambda v: f"median {statistics.median(v) * 1e3:9.3f} ms  (min {min(v) * 1e3:.3f}, max {max(v) * 1e3:.3f}; n = {len(v)})"
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {d['n_reads']} reads, {d['n_rec']} records, query column sorted: {'yes' if d['sorted_queries'] else 'no'}; "
        f"strand drawn at random; device {d['device']}")
    say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream around the call's launches; device form, "
        f"max_overhang = {H}, min_ratio = {F}, symmetric = 1; a process per build of libraft_hip_cc.so")
    same = True
    for name, r in runs:
        say(f"build: {name}")
        for key, label in (("proper", "PROPER (kinds 2..5)"), ("all", "ALL (kinds 1..5)")):
            s = r[key + "_summary"]
            say(f"  raft_hip_components_device, {label:20s} {ms(r[key])}  launches = {s['launches']}")
            say(f"    edges = {s['edge_records']}, components = {s['components']}, singletons = {s['singletons']}, largest = {s['largest_reads']} reads "
                f"({s['reads_in_largest_permille']} per mille), checksum = {s['checksum']}")
            say(f"    25 B per record streamed: {25 * r['n_rec'] / 1e9:.3f} GB, {25 * r['n_rec'] / statistics.median(r[key]) / 1e12:.2f} TB/s over the whole call")
        say(f"  the same call without records (every launch but the link kernel, a forest of roots)  {ms(r['no_records'])}")
        say(f"  yardstick: raft_hip_overlap_ends_device, same stream, same H and F  {ms(r['ends'])};  components (PROPER) / overlap_ends = "
            f"{statistics.median(r['proper']) / statistics.median(r['ends']):.2f}")
        s = r["proper_summary"]
        same = same and counts == [r["n_rec"], s["edge_records"], s["components"], s["largest_reads"], s["checksum"]]
    mp = statistics.median(d["proper"])
    say(f"host walk (tools/components_walk, one thread, -O2, PROPER)  median {statistics.median(host_s):8.3f} s  (min {min(host_s):.3f}, max {max(host_s):.3f}; "
        f"n = {len(host_s)})  walk / device call = {statistics.median(host_s) / mp:.0f}")
    say(f"the walk's counts and checksum equal the device's in every build: {'yes' if same else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
