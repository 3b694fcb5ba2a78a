#!/usr/bin/env python3
"""Device time of raft_hip_best_overlaps_device on a synthetic stream of the bench's record count (GPU box).

  python tools/best_overlaps_probe.py [--reads N] [--out profiles/best_overlaps_timing.txt]

One process under its own time limit; if it fails or runs out of time the probe ends, and nothing more is started on the device.
In it: the set of bench.py's default workload resident in HBM with all six record columns, a strand byte per record drawn at random,
H = 1000 and F = 800, and as ``skip`` the reads raft_hip_overlap_ends_device finds contained in the same process; kernel_seconds of
raft_hip_best_overlaps_device -- HIP events on the context's stream around the clear of the table and the three launches -- under
symmetric = 0 and 1, each the median of 10 calls after 2 warm ones; beside it the same for raft_hip_overlap_ends_device without the
kind bytes under the same symmetric flag IN THE SAME PROCESS: the yardstick, one stream of the same 25 B per record with the same two
gathers.

Bytes, the model of DESIGN.md I.18: per record 25 in (six columns and the strand byte) and two 4-byte digest gathers (served from the
cache for a sorted query column); per read 4 B of length and 1 B of skip in and 4 B of digest out, 16 B of table cleared, and in the
pairs kernel 16 B of table and 4 B of digest in, up to two 8-byte partner slots gathered, 17 B out.  The atomics: at most one 8-byte
maximum per run, wave and end on the query side, one per candidate that can still win on the target side."""
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
        ends, te = times(lambda: eng.overlap_ends(*cols, strand, max_overhang=1000, min_ratio_permille=800, symmetric=symmetric),
                         lambda: eng.last_overlap_ends_seconds)
        skip = torch.from_numpy((ends["status"] == engine.END_READ_CONTAINED).astype("uint8")).to(dev)
        got, tb = times(lambda: eng.best_overlaps(*cols, strand, max_overhang=1000, min_ratio_permille=800, symmetric=symmetric, skip=skip),
                        lambda: eng.last_best_overlaps_seconds)
        views = 1 if symmetric else 2
        assert got["n_records"] == n_rec and got["candidates"] + got["left_out"] == views * (ends["kind_end3"] + ends["kind_end5"])
        assert got["reads_skipped"] == ends["reads_contained"] == int(skip.sum()) and got["ends_mutual"] % 2 == 0
        assert int((got["partner"] >= 0).sum()) == got["ends_best"] == int((got["span"] > 0).sum())
        out["runs"].append({"symmetric": int(symmetric), "ends": te, "best": tb, "summary": {k: got[k] for k, _ in engine._BestSummary._fields_}})
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_overlaps_timing.txt"))
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
    n, n_reads = res["n_rec"], res["n_reads"]
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {n_reads} reads, {n} records; device {res['device']}")
    say(f"method: one process; in it {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; device form, max_overhang = 1000, "
        "min_ratio_permille = 800, a strand byte per record drawn at random, skip = the reads overlap_ends finds contained; the yardstick "
        "raft_hip_overlap_ends_device without the kind bytes under the same symmetric flag in the same process")
    for run in res["runs"]:
        my, mb = statistics.median(run["ends"]), statistics.median(run["best"])
        stream, per_read = n * 25, n_reads * (5 + 4 + 16 + 20 + 17)
        say(f"symmetric = {run['symmetric']}  ({', '.join(f'{k} = {v}' for k, v in run['summary'].items())})")
        say(f"  yardstick: raft_hip_overlap_ends_device   median {my * 1e3:8.3f} ms  (min {min(run['ends']) * 1e3:.3f}, max {max(run['ends']) * 1e3:.3f}; "
            f"n = {len(run['ends'])})  25 B per record  {stream / 1e9:7.3f} GB  {stream / my / 1e12:5.2f} TB/s = {100 * stream / my / PEAK:4.1f} % of 8 TB/s")
        say(f"  raft_hip_best_overlaps_device             median {mb * 1e3:8.3f} ms  (min {min(run['best']) * 1e3:.3f}, max {max(run['best']) * 1e3:.3f}; "
            f"n = {len(run['best'])})  25 B per record + {per_read // n_reads} B per read  {(stream + per_read) / 1e9:7.3f} GB  "
            f"{(stream + per_read) / mb / 1e12:5.2f} TB/s = {100 * (stream + per_read) / mb / PEAK:4.1f} % of 8 TB/s;  time / overlap_ends time = {mb / my:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
