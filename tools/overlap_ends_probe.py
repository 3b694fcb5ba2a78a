#!/usr/bin/env python3
"""Device time of raft_hip_overlap_ends_device on a synthetic stream of the bench's record count (GPU box).

  python tools/overlap_ends_probe.py [--reads N] [--out profiles/overlap_ends_timing.txt]

One process under its own time limit; if it fails or runs out of time the probe ends, and nothing more is started on the device.
In it: the set of bench.py's default workload resident in HBM with all six record columns, a strand byte per record drawn at random,
H = 1000 and F = 800; kernel_seconds of raft_hip_overlap_ends_device -- HIP events on the context's stream around its launches --
with and without the kind bytes, under symmetric = 0 and 1, each the median of 10 calls after 2 warm ones; beside it the same for
raft_hip_census_device under the same symmetric flag IN THE SAME PROCESS: the yardstick, the kernel whose shape this one has.

Bytes per record, the model of DESIGN.md I.17: 25 in (six columns and the strand byte), 1 out with the kind bytes; on top the two
length gathers per record (8 B asked for, served from the cache for a sorted query column) and the adds, at most one per record and
side after joining.  The census moves 24 B per record (16 when symmetric: it does not read ts / te) and gathers lengths for its few
containment candidates only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12          # bytes per second: the device's HBM


def child(args):
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
    gen.manual_seed(7)
    strand = (torch.rand(n_rec, device=dev, generator=gen) < 0.5).to(torch.uint8)

    def times(call, seconds):
        t, res = [], None
        for i in range(args.warm + args.calls):
            res = call()
            if i >= args.warm:
                t.append(seconds())
        return res, t

    out = {"n_reads": n_reads, "n_rec": n_rec, "device": torch.cuda.get_device_name(0), "runs": []}
    for symmetric in (False, True):
        _, tc = times(lambda: eng.census(*cols, symmetric=symmetric), lambda: eng.last_census_seconds)
        run = {"symmetric": int(symmetric), "census": tc}
        for kinds in (False, True):
            got, te = times(lambda: eng.overlap_ends(*cols, strand, max_overhang=1000, min_ratio_permille=800, symmetric=symmetric, kinds=kinds),
                            lambda: eng.last_overlap_ends_seconds)
            by_kind = [got[k] for k in ("kind_invalid", "kind_internal", "kind_query_contained", "kind_target_contained", "kind_end3", "kind_end5", "kind_self")]
            assert sum(by_kind) == n_rec == got["n_records"]
            assert int(got["counts"].sum()) == (1 if symmetric else 2) * sum(by_kind[1:6])
            if kinds:
                assert torch.bincount(got["kinds"].to(torch.int64), minlength=7).tolist() == by_kind
                del got["kinds"]
            run["kinds" if kinds else "plain"] = te
            run["by_kind"] = by_kind
        out["runs"].append(run)
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_ends_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-limit", type=int, default=300, help="seconds the process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reads", str(args.reads), "--calls", str(args.calls), "--warm", str(args.warm)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
    except subprocess.TimeoutExpired:
        say(f"not through after {args.step_limit} s; the probe ends here")
        return 1
    found = [ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")]
    if r.returncode != 0 or len(found) != 1:
        say(f"exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}")
        return 1
    res = json.loads(found[0][7:])
    n = res["n_rec"]
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {res['n_reads']} reads, {n} records; device {res['device']}")
    say(f"method: one process; in it {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; device form, max_overhang = 1000, "
        "min_ratio_permille = 800, a strand byte per record drawn at random; the census under the same symmetric flag in the same process")
    for run in res["runs"]:
        cen_bytes = n * (16 if run["symmetric"] else 24)
        mc = statistics.median(run["census"])
        say(f"symmetric = {run['symmetric']}  (records by kind 0..6: {run['by_kind']})")
        say(f"  yardstick: raft_hip_census_device   median {mc * 1e3:8.3f} ms  (min {min(run['census']) * 1e3:.3f}, max {max(run['census']) * 1e3:.3f}; "
            f"n = {len(run['census'])})  {cen_bytes / 1e9:7.3f} GB  {cen_bytes / mc / 1e12:5.2f} TB/s = {100 * cen_bytes / mc / PEAK:4.1f} % of 8 TB/s")
        for key, per_record, what in (("plain", 25, "without the kind bytes"), ("kinds", 26, "with the kind bytes   ")):
            t = run[key]
            m = statistics.median(t)
            b = n * per_record
            say(f"  raft_hip_overlap_ends_device {what} median {m * 1e3:8.3f} ms  (min {min(t) * 1e3:.3f}, max {max(t) * 1e3:.3f}; n = {len(t)})  "
                f"{per_record} B per record  {b / 1e9:7.3f} GB  {b / m / 1e12:5.2f} TB/s = {100 * b / m / PEAK:4.1f} % of 8 TB/s;  time / census time = {m / mc:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
