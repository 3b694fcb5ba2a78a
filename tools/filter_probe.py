#!/usr/bin/env python3
"""Device time of raft_hip_filter_overlaps_device on a synthetic stream of the bench's record count (GPU box).

  python tools/filter_probe.py [--reads N] [--out profiles/filter_timing.txt]

Three steps, one per keep share (100 %, 50 %, 0 %), each a process of its own under its own time limit; a step that fails or runs
out of time ends the probe, and nothing more is started on the device.  In a step: the set of bench.py's default workload resident in
HBM with all six record columns, two quality columns made for the share (block = 1000, matches = 999 on a kept record, 990 on a
dropped one, P = 995 per mille; the kept records are drawn at random), kernel_seconds of one raft_hip_filter_overlaps_device call --
HIP events on the context's stream around its clears and launches -- as the median of 10 calls after 2 warm ones, beside the same for
raft_hip_census_device with symmetric = 0 on the same columns IN THE SAME PROCESS: the yardstick, an existing kernel that streams the
same columns with the same loads.

Bytes per record.  The model of DESIGN.md I.16: 24 (the flag kernel's six columns) + 24 1/8 (the scatter kernel's six columns and
the bitmap) + 24 k (the kept records written, k the kept share), plus 8 when P > 0.  As built, the flag kernel reads qs, qe, ts, te
and, when P > 0, matches and block (16 + 8), not the two id columns, and a lane of the scatter kernel whose four records are all
dropped loads nothing: the figure "as built" counts 24 1/8 + 1/8 + 24 g + 24 k, g the share of lanes with a kept record.  Both are
set against the time; the census moves 24 bytes per record."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHARES = (100, 50, 0)
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
    gen.manual_seed(args.child)
    keep = torch.rand(n_rec, device=dev, generator=gen) * 100 < args.child
    matches = eng.device_copy(torch.where(keep, 999, 990).to(torch.int32))
    block = eng.device_copy(torch.full((n_rec,), 1000, dtype=torch.int32, device=dev))
    lanes = float(torch.nn.functional.pad(keep, (0, -n_rec % 4)).view(-1, 4).any(dim=1).float().mean()) if n_rec else 0.0
    out = [eng.device_tensor(n_rec, torch.int32) for _ in range(6)]

    def times(call, seconds):
        t, res = [], None
        for i in range(args.warm + args.calls):
            res = call()
            if i >= args.warm:
                t.append(seconds())
        return res, t

    _, tc = times(lambda: eng.census(*cols, symmetric=False), lambda: eng.last_census_seconds)
    got, tf = times(lambda: eng.filter_overlaps(*cols[1:], matches, block, min_identity_permille=995, out=out), lambda: eng.last_filter_overlaps_seconds)
    assert got["n_kept"] == int(keep.sum()) and got["below_identity"] == n_rec - got["n_kept"] and got["below_span"] == 0
    if got["n_kept"]:
        at = torch.nonzero(keep)[:: max(got["n_kept"] // 1000, 1), 0]              # a thousand kept records, where they must be
        rank = torch.cumsum(keep, 0)[at] - 1
        assert all(bool((o_[rank] == c[at]).all()) for o_, c in zip(out, cols[1:]))
    eng.close()
    print("RESULT " + json.dumps({"share": args.child, "n_reads": n_reads, "n_rec": n_rec, "n_kept": got["n_kept"], "lanes": lanes, "census": tc, "filter": tf,
                                  "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-limit", type=int, default=240, help="seconds one step may take")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child >= 0:
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    results = []
    for share in SHARES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(share), "--reads", str(args.reads), "--calls", str(args.calls), "--warm", str(args.warm)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_limit)
        except subprocess.TimeoutExpired:
            say(f"step {share} %: not through after {args.step_limit} s; the probe ends here")
            return 1
        found = [ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")]
        if r.returncode != 0 or len(found) != 1:
            say(f"step {share} %: exit status {r.returncode}; the probe ends here\n{r.stdout[-2000:]}")
            return 1
        results.append(json.loads(found[0][7:]))
    r0 = results[0]
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {r0['n_reads']} reads, {r0['n_rec']} records; device {r0['device']}")
    say(f"method: a process per keep share; in it {args.calls} calls after {args.warm} warm ones, HIP events on the context's stream; device form, "
        "min_identity_permille = 995, min_span = 0, the kept records drawn at random; the census with symmetric = 0 in the same process")
    for r in results:
        n, k = r["n_rec"], r["n_kept"] / max(r["n_rec"], 1)
        mc, mf = statistics.median(r["census"]), statistics.median(r["filter"])
        model, built = n * (24 + 24.125 + 24 * k + 8), n * (24.125 + 0.125 + 24 * r["lanes"] + 24 * k)
        say(f"keep share {r['share']:3d} % ({r['n_kept']} kept, {100 * r['lanes']:.1f} % of the lanes hold a kept record)")
        say(f"  yardstick: raft_hip_census_device, symmetric = 0   median {mc * 1e3:8.3f} ms  (min {min(r['census']) * 1e3:.3f}, max {max(r['census']) * 1e3:.3f}; "
            f"n = {len(r['census'])})  {n * 24 / 1e9:7.3f} GB  {n * 24 / mc / 1e12:5.2f} TB/s = {100 * n * 24 / mc / PEAK:4.1f} % of 8 TB/s")
        say(f"  raft_hip_filter_overlaps_device (flag, scan, scatter) median {mf * 1e3:8.3f} ms  (min {min(r['filter']) * 1e3:.3f}, max {max(r['filter']) * 1e3:.3f}; "
            f"n = {len(r['filter'])})")
        say(f"    model    {model / n:6.3f} B per record  {model / 1e9:7.3f} GB  {model / mf / 1e12:5.2f} TB/s = {100 * model / mf / PEAK:4.1f} % of 8 TB/s;  "
            f"rate / census rate = {model / mf / (n * 24 / mc):.2f}")
        say(f"    as built {built / n:6.3f} B per record  {built / 1e9:7.3f} GB  {built / mf / 1e12:5.2f} TB/s = {100 * built / mf / PEAK:4.1f} % of 8 TB/s;  "
            f"rate / census rate = {built / mf / (n * 24 / mc):.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
