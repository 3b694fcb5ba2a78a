#!/usr/bin/env python3
"""Device time of raft_hip_lift_overlaps_device on the bench's set against the same rule walked on one host core (GPU box).

  python tools/lift_probe.py [--reads N] [--out profiles/fragment_paf_timing.txt]

Two steps, each a process of its own under its own time limit; a step that fails or runs out of time ends the probe, and nothing more
is started on the device.  Step "device": the set of bench.py's default workload resident in HBM with its six record columns and a
strand column drawn at random; one pass of the context, whose own fragment table the lift then reads (fragments=None); kernel_seconds
of the size query -- the digest, count and scan launches -- and of the filling call -- those and the fill launch --, HIP events on the
context's stream, each as the median of 10 calls after 2 warm ones; beside them, in the same process, raft_hip_filter_overlaps_device
with both rules off (every record kept): the yardstick, a compaction that streams the same six columns with the same loads and
writes six where this writes eight.  The share of records on the fast path is counted with torch.  The step leaves the columns and
the table in a file for step "walk": tools/lift_walk (built here with g++ -O2 if it is not there), one host thread, 3 repeats; its
counts and its checksum over all outputs must equal the device's.

Bytes.  Streamed: 25 per record in the count kernel (six int32 columns and the strand byte), 25 more in the fill kernel for every
lane with an output, 29 per output written (the lane counts between the two kernels, a byte per record each way, are not counted).  Gathered: two 16-byte digests per record in either kernel (the digest array is 16 B per
read: cache-resident at this size), and the rows of the records off the fast path.  The streamed bytes are set against the time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12          # bytes per second: the device's HBM
WALK = os.path.join(ROOT, "tools", "lift_walk")


def child(args):
    import numpy as np
    import torch

    from bench import DEFAULT_READS, WORKLOADS
    from raft_amd import engine
    from raft_amd.params import RaftParams
    from raft_amd.synth import make_overlaps

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
    eng.run_device(*cols)
    s = eng.finish()
    table = eng.fetch()
    off, fb, fe = (torch.from_numpy(np.ascontiguousarray(table[k])).to(dev) for k in ("frag_offset", "frag_begin", "frag_end"))

    # the fast path: both reads have one row and neither side leaves it
    rows = off[1:] - off[:-1]
    qid, qs, qe, tid, ts, te = cols[1:]

    def inside(ids, a, b):
        ids = ids.long()
        first = off[:-1][ids].clamp(max=max(fb.numel() - 1, 0))
        return (rows[ids] == 1) & (a >= fb[first]) & (b <= fe[first])
    fast = int(((qid != tid) & (qe > qs) & (te > ts) & inside(qid, qs, qe) & inside(tid, ts, te)).sum())
    del rows
    torch.cuda.empty_cache()

    lib = engine.load_side_library("lift")
    import ctypes as C
    records = engine._Records(n_rec, *[c.data_ptr() for c in cols[1:]])
    own = engine._FragTable(-1, 0, 0, 0)
    sm, err, secs = engine._LiftSummary(), C.c_int64(-1), C.c_double(0.0)

    def call(cap, outs):
        rc = lib.raft_hip_lift_overlaps_device(eng._ctx, n_reads, C.byref(records), C.c_void_p(strand.data_ptr()), C.byref(own), 1, cap,
                                               *[C.c_void_p(t.data_ptr() if t is not None else 0) for t in outs], C.byref(sm), C.byref(err), C.byref(secs))
        eng._check(rc, err.value)
        return secs.value

    def times(fn):
        t = []
        for i in range(args.warm + args.calls):
            v = fn()
            if i >= args.warm:
                t.append(v)
        return t

    head = times(lambda: call(0, [None] * 8))
    n_out = int(sm.n_out)
    outs = [eng.device_tensor(max(n_out, 1), torch.uint8 if k == 6 else torch.int32) for k in range(8)]
    full = times(lambda: call(n_out, outs))
    summary = {k: int(getattr(sm, k)) for k, _ in sm._fields_}
    checksum = int(sum(int(t[:n_out].sum(dtype=torch.int64)) for t in outs[:6]))

    def flt():
        eng.filter_overlaps(*cols[1:], out=flt_out)
        return eng.last_filter_overlaps_seconds
    flt_out = [eng.device_tensor(n_rec, torch.int32) for _ in range(6)]
    tf = times(flt)

    with open(args.dump, "wb") as f:
        np.array([n_reads, fb.numel(), n_rec, 1], np.int64).tofile(f)
        for a in (table["frag_offset"].astype(np.int64), table["frag_begin"].astype(np.int32), table["frag_end"].astype(np.int32)):
            np.ascontiguousarray(a).tofile(f)
        for t in cols[1:] + [strand]:
            t.cpu().numpy().tofile(f)
    eng.close()
    print("RESULT " + json.dumps({"n_reads": n_reads, "n_rec": n_rec, "n_frag": int(s.n_fragments), "fast": fast, "summary": summary, "checksum": checksum,
                                  "head": head, "full": full, "filter": tf, "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fragment_paf_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-limit", type=int, default=300, help="seconds one step may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dump", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if not os.path.exists(WALK):
        subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "lift_walk.cpp"), "-o", WALK], check=True)
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "set.bin")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dump", dump, "--reads", str(args.reads), "--calls", str(args.calls), "--warm", str(args.warm)]
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
        print("device step done; the host walk runs", flush=True)
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
    counts, host_s = [int(x) for x in f[1:8]], [float(x) for x in f[8:]]
    sm = d["summary"]
    same = counts == [d["n_rec"], sm["n_out"], sm["records_none"], sm["records_cut"], sm["pairs_dropped"], sm["most_per_record"], d["checksum"]]
    n, n_out = d["n_rec"], sm["n_out"]
    mh, mf, mflt = statistics.median(d["head"]), statistics.median(d["full"]), statistics.median(d["filter"])
    streamed = n * 25 * 2 + n_out * 29
    flt_bytes = n * (16 + 24.125 + 24)
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {d['n_reads']} reads, {n} records, the context's own fragment table ({d['n_frag']} rows); strand drawn at random; "
        f"device {d['device']}")
    say(f"method: {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; device form, min_len = 1, fragments = the finished pass's")
    say(f"outputs: n_out = {n_out}, n_out / n_rec = {n_out / max(n, 1):.4f}; records on the fast path {d['fast']} = {100 * d['fast'] / max(n, 1):.2f} %; "
        f"cut {sm['records_cut']}, without a fragment pair {sm['records_none']}, dropped pairs {sm['pairs_dropped']}, most from one record {sm['most_per_record']}")
    say(f"  size query (clear, digest, count, scan)      median {mh * 1e3:8.3f} ms  (min {min(d['head']) * 1e3:.3f}, max {max(d['head']) * 1e3:.3f}; n = {len(d['head'])})")
    say(f"  filling call (the same and the fill launch)  median {mf * 1e3:8.3f} ms  (min {min(d['full']) * 1e3:.3f}, max {max(d['full']) * 1e3:.3f}; n = {len(d['full'])})"
        f"  -> fill {1e3 * (mf - mh):.3f} ms")
    say(f"    streamed {streamed / max(n, 1):6.2f} B per record  {streamed / 1e9:7.3f} GB  {streamed / mf / 1e12:5.2f} TB/s = {100 * streamed / mf / PEAK:4.1f} % of 8 TB/s"
        f"  (gathered beside them: {n * 64 / 1e9:.3f} GB of digests, cache-resident)")
    say(f"  yardstick: raft_hip_filter_overlaps_device, every record kept  median {mflt * 1e3:8.3f} ms  (min {min(d['filter']) * 1e3:.3f}, max {max(d['filter']) * 1e3:.3f}; "
        f"n = {len(d['filter'])})  {flt_bytes / 1e9:7.3f} GB  {flt_bytes / mflt / 1e12:5.2f} TB/s;  lift / filter = {mf / mflt:.2f}")
    say(f"  host walk (tools/lift_walk, one thread, -O2, the brute-force rule)  median {statistics.median(host_s):8.3f} s  (min {min(host_s):.3f}, max {max(host_s):.3f}; "
        f"n = {len(host_s)})  walk / filling call = {statistics.median(host_s) / mf:.0f}")
    say(f"  the walk's counts and checksum equal the device's: {'yes' if same else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
