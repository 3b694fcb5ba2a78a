#!/usr/bin/env python3
"""Device time of raft_hip_string_graph_device against the same rule walked sequentially on one host core (GPU box), on two sets: the
bench's, which is sparse in dovetails between reads that stay, and a layout set -- reads laid on a line with random strands and exact
coordinates, every pair that shares 500 bases a record and its mirror --, whose records are mostly dovetails.

  python tools/string_graph_probe.py [--reads N] [--layout-records M] [--out profiles/string_graph_timing.txt]

Steps, each a process of its own under its own time limit; a step that fails or runs out of time ends the probe, and nothing more is
started on the device.  Step "device" (once per set): the set resident in HBM, the contained reads of raft_hip_overlap_ends_device as
the skip bytes; kernel_seconds of the whole call -- HIP events on the context's stream around its launches -- as the median of
``--calls`` calls after ``--warm`` warm ones, at fuzz 1000; beside it, in the same process, raft_hip_overlap_ends_device, which streams
the same 25 B per record.  The step leaves the arrays in a file for step "walk": tools/string_graph_walk (built here with g++ -O2 if it
is not there), one host thread; its counts and its checksum over kept[] must equal the device's.  The kernels one by one are a kernel
trace's business, in a run of its own: --trace SET runs that set's device step alone, two calls, for a profiler to wrap."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WALK = os.path.join(ROOT, "tools", "string_graph_walk")
H, F, Z = 1000, 800, 1000


def layout_set(n_reads, dev, gen):
    """Reads on a line, every pair within six places that shares 500 bases or more as a record and its mirror -> read_len, six columns, strand"""
    import torch
    length = torch.randint(9000, 11001, (n_reads,), device=dev, generator=gen, dtype=torch.int64)
    pos = torch.cumsum(torch.randint(1500, 2501, (n_reads,), device=dev, generator=gen, dtype=torch.int64), 0)
    orient = torch.randint(0, 2, (n_reads,), device=dev, generator=gen, dtype=torch.int64)
    ids = torch.randperm(n_reads, device=dev, generator=gen)             # the read at each place
    parts = []
    for k in range(1, 7):
        i = torch.arange(n_reads - k, device=dev)
        j = i + k
        d = pos[j] - pos[i]
        end = torch.minimum(length[i], d + length[j])
        keep = end - d >= 500
        i, j, d, end = i[keep], j[keep], d[keep], end[keep]
        a0, a1, b0, b1 = d, end, torch.zeros_like(d), end - d
        fa, fb = orient[i] != 0, orient[j] != 0
        a0, a1 = torch.where(fa, length[i] - a1, a0), torch.where(fa, length[i] - a0, a1)
        b0, b1 = torch.where(fb, length[j] - b1, b0), torch.where(fb, length[j] - b0, b1)
        rev = (orient[i] != orient[j]).to(torch.uint8)
        parts.append((ids[i], a0, a1, ids[j], b0, b1, rev))
        parts.append((ids[j], b0, b1, ids[i], a0, a1, rev))
    cols = [torch.cat([p[c] for p in parts]) for c in range(7)]
    order = torch.argsort(cols[0], stable=True)                          # grouped by query, as an overlapper writes
    read_len = torch.empty(n_reads, dtype=torch.int32, device=dev)
    read_len[ids] = length.to(torch.int32)
    return read_len, [c[order].to(torch.int32).contiguous() for c in cols[:6]], cols[6][order].contiguous()


def child(args):
    import numpy as np
    import torch

    from bench import DEFAULT_READS, WORKLOADS
    from raft_amd import engine
    from raft_amd.params import RaftParams
    from raft_amd.synth import make_overlaps

    if args.sg_lib:
        engine._SIDE_LATER["sg"] = (os.path.abspath(args.sg_lib),) + engine._SIDE_LATER["sg"][1:]
    dev = "cuda:0"
    gen_kw, est_cov, _ = WORKLOADS["hg002"]
    eng = engine.Engine(RaftParams(est_cov=est_cov), device=0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    if args.set == "bench":
        n_reads = args.reads or DEFAULT_READS["hg002"]
        o = make_overlaps(n_reads, seed=20241008, device=dev, **gen_kw)
        tensors = [t.contiguous() for t in (o.read_len,) + tuple(o.columns())]
        strand = (torch.rand(o.n_rec, device=dev, generator=gen) < 0.5).to(torch.uint8)
        del o
    else:
        n_reads = max(8, args.layout_records // 9)
        read_len, six, strand = layout_set(n_reads, dev, gen)
        tensors = [read_len] + six
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

    ends = eng.overlap_ends(*cols, strand, max_overhang=H, min_ratio_permille=F, symmetric=True)
    skip_host = (np.asarray(ends["status"]) == engine.END_READ_CONTAINED).astype(np.uint8)
    skip = eng.device_copy(torch.from_numpy(skip_host).to(dev))
    last = {}

    def graph():
        last["r"] = eng.string_graph(*cols, strand, max_overhang=H, min_ratio_permille=F, fuzz=Z, symmetric=True, skip=skip)
        return last["r"]["kernel_seconds"]

    def ends_time():
        eng.overlap_ends(*cols, strand, max_overhang=H, min_ratio_permille=F, symmetric=True)
        return eng.last_overlap_ends_seconds
    out = {"set": args.set, "n_reads": n_reads, "n_rec": n_rec, "device": torch.cuda.get_device_name(0), "graph": times(graph), "ends": times(ends_time)}
    r = last["r"]
    weights = (np.arange(2 * n_reads, dtype=np.int64) & 1023) + 1
    out["summary"] = dict(r["summary"], checksum=int((r["kept"].reshape(-1).astype(np.int64) * weights).sum()), launches=r["launches"])
    if args.dump:
        with open(args.dump, "wb") as f:
            np.array([n_reads, n_rec, H, F, Z, 1], np.int64).tofile(f)
            for t in cols + [strand]:
                t.cpu().numpy().tofile(f)
            skip_host.tofile(f)
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="reads of the bench's set; 0 = the bench's default size")
    ap.add_argument("--layout-records", type=int, default=0, help="records of the layout set, about; 0 = as many as the bench's set has")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_graph_timing.txt"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--walks", type=int, default=1, help="repeats of the host walk")
    ap.add_argument("--step-limit", type=int, default=300, help="seconds one step may take")
    ap.add_argument("--trace", default="", choices=["", "bench", "layout"], help="that set's device step alone, in this process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--set", default="bench", help=argparse.SUPPRESS)
    ap.add_argument("--dump", default="", help=argparse.SUPPRESS)
    ap.add_argument("--sg-lib", default="", help=argparse.SUPPRESS)
    ap.add_argument("--other-lib", default="", help="a second build of libraft_hip_sg.so, timed as well on both sets")
    ap.add_argument("--other-name", default="the other build", help="what that build is")
    args = ap.parse_args()
    if args.child or args.trace:
        if args.trace:
            args.set, args.calls, args.warm = args.trace, 2, 1
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if not os.path.exists(WALK):
        subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "string_graph_walk.cpp"), "-o", WALK], check=True)
    ms = lambda v: f"median {statistics.median(v) * 1e3:9.3f} ms  (min {min(v) * 1e3:.3f}, max {max(v) * 1e3:.3f}; n = {len(v)})"
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream around the call's launches (two spans: the call "
        f"waits once for the number of views); device form, max_overhang = {H}, min_ratio = {F}, fuzz = {Z}, symmetric = 1, skip = the reads "
        "overlap_ends finds contained; a process per set")
    same, layout_records = True, args.layout_records
    with tempfile.TemporaryDirectory() as tmp:
        for which in ("bench", "layout"):
            dump = os.path.join(tmp, f"{which}.bin")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--set", which, "--reads", str(args.reads), "--layout-records", str(layout_records),
                   "--calls", str(args.calls), "--warm", str(args.warm), "--dump", dump]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
            except subprocess.TimeoutExpired:
                say(f"step device ({which}): not through after {args.step_limit} s; the probe ends here")
                return 1
            found = [ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")]
            if r.returncode != 0 or len(found) != 1:
                say(f"step device ({which}): exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}")
                return 1
            d = json.loads(found[0][7:])
            print(f"device step done: {which}", flush=True)
            if which == "bench" and not layout_records:
                layout_records = d["n_rec"]
            try:
                w = subprocess.run([WALK, dump, str(args.walks)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
            except subprocess.TimeoutExpired:
                say(f"step walk ({which}): not through after {args.step_limit} s; the probe ends here")
                return 1
            os.remove(dump)
            walk = [ln for ln in w.stdout.split("\n") if ln.startswith("WALK ")]
            if w.returncode != 0 or len(walk) != 1:
                say(f"step walk ({which}): exit status {w.returncode}; the probe ends here\n{w.stdout[-2000:]}")
                return 1
            f = walk[0].split()
            counts, host_s = [int(x) for x in f[1:7]], [float(x) for x in f[7:]]
            s = d["summary"]
            what = "bench.py workload hg002, strand drawn at random" if which == "bench" else "layout on a line, six places deep, every record with its mirror"
            say(f"set `{which}`: {what}; {d['n_reads']} reads, {d['n_rec']} records; device {d['device']}")
            say(f"  raft_hip_string_graph_device  {ms(d['graph'])}  launches = {s['launches']}")
            say(f"    dovetail views = {s['dovetail_views']} ({1000 * s['dovetail_views'] // max(d['n_rec'], 1)} per mille of the records), left out = "
                f"{s['views_left_out']}, arcs = {s['arcs']}, reducible = {s['reducible_arcs']}, edges = {s['edges']}, kept = {s['kept_edges']}, "
                f"longest row = {s['longest_row']}, reads left out = {s['reads_flagged']}, checksum = {s['checksum']}")
            say(f"  yardstick: raft_hip_overlap_ends_device, same stream, same H and F  {ms(d['ends'])};  string_graph / overlap_ends = "
                f"{statistics.median(d['graph']) / statistics.median(d['ends']):.2f}")
            say(f"  host walk (tools/string_graph_walk, one thread, -O2)  median {statistics.median(host_s):8.3f} s  (n = {len(host_s)})  walk / device call = "
                f"{statistics.median(host_s) / statistics.median(d['graph']):.0f}")
            ok = counts == [d["n_rec"], s["dovetail_views"], s["arcs"], s["reducible_arcs"], s["kept_edges"], s["checksum"]]
            say(f"  the walk's counts and checksum equal the device's: {'yes' if ok else 'NO ' + str(counts)}")
            same = same and ok
            if args.other_lib:
                try:
                    r = subprocess.run(cmd[:-2] + ["--sg-lib", args.other_lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
                except subprocess.TimeoutExpired:
                    say(f"step device ({which}, {args.other_name}): not through after {args.step_limit} s; the probe ends here")
                    return 1
                found = [ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")]
                if r.returncode != 0 or len(found) != 1:
                    say(f"step device ({which}, {args.other_name}): exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}")
                    return 1
                o = json.loads(found[0][7:])
                agrees = o["summary"]["checksum"] == s["checksum"] and o["summary"]["kept_edges"] == s["kept_edges"]
                say(f"  the other build, {args.other_name}:  {ms(o['graph'])}  launches = {o['summary']['launches']};  the same graph: {'yes' if agrees else 'NO'}")
                same = same and agrees
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
