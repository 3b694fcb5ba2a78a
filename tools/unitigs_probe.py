#!/usr/bin/env python3
"""Device time of raft_hip_unitigs_device at the bench's read count, beside a plain sequential walk on one host thread (GPU box).

  python tools/unitigs_probe.py [--reads N] [--out profiles/unitigs_timing.txt]

One process under its own time limit; if it fails or runs out of time the probe ends, and nothing more is started on the device.
In it two tables over the same reads:
  * "stream": the set of bench.py's default workload with a strand byte per record drawn at random, through
    raft_hip_overlap_ends_device (H = 1000, F = 800) and raft_hip_best_overlaps_device with the contained reads left out -- the
    table a user has;
  * "chains": made directly -- a random permutation of the reads cut into chains of ``--chain`` reads on random strands, every
    tenth closed to a cycle -- the table a well-connected set would give, and the one that makes the cycle pass run.
Per table kernel_seconds of raft_hip_unitigs_device (HIP events on the context's stream around the launches, the host's look at the
control words between the ranking and the rest not included), the median of ``--calls`` calls after ``--warm`` warm ones, and the
seconds of tools/unitig_walk.cpp (g++ -O2, one thread, the consistency check and every output array included) on the same arrays,
the median of three.  The walk is the figure to compare with: it was measured, the same day, on the host of the same machine."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WALK = os.path.join(ROOT, "build", "tools", "unitig_walk")
WALK_SRC = os.path.join(ROOT, "tools", "unitig_walk.cpp")


def build_walk():
    if not os.path.exists(WALK) or os.path.getmtime(WALK) < os.path.getmtime(WALK_SRC):
        os.makedirs(os.path.dirname(WALK), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", WALK_SRC, "-o", WALK], check=True)


def chains_table(rng, read_len, chain):
    """numpy: partner [n, 2], span [n, 2], flags of chains of ``chain`` reads over a permutation, every tenth a cycle"""
    import numpy as np
    n = read_len.size
    perm = rng.permutation(n).astype(np.int64)
    pos = np.arange(n)
    first = pos - pos % chain
    last = np.minimum(first + chain - 1, n - 1)
    closes = (pos == last) & ((pos // chain) % 10 == 0) & (last > first)
    nxt = np.where(pos < last, pos + 1, np.where(closes, first, -1))
    o = rng.integers(0, 2, n)
    m = nxt >= 0
    a, b = perm[pos[m]], perm[nxt[m]]
    e_out, e_in = 1 - o[pos[m]], o[nxt[m]]
    rev = (e_in == e_out).astype(np.int64)
    s = 1 + (rng.integers(0, 2 ** 31, a.size) % np.minimum(read_len[a], read_len[b]).astype(np.int64))
    partner, span, flags = np.full((n, 2), -1, np.int32), np.zeros((n, 2), np.int32), np.zeros(n, np.int64)
    for r, e, p in ((a, e_out, b), (b, e_in, a)):
        partner[r, e], span[r, e] = p, s
        np.bitwise_or.at(flags, r, (2 | rev) << (2 * e))
    return partner, span, flags.astype(np.uint8)


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
    cols = [eng.device_copy(t.contiguous()) for t in (o.read_len,) + tuple(o.columns())]
    n_rec = o.n_rec
    del o
    torch.cuda.empty_cache()
    eng.use_torch_stream()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    strand = (torch.rand(n_rec, device=dev, generator=gen) < 0.5).to(torch.uint8)
    ends = eng.overlap_ends(*cols, strand, max_overhang=1000, min_ratio_permille=800)
    skip = torch.from_numpy((ends["status"] == engine.END_READ_CONTAINED).astype("uint8")).to(dev)
    best = eng.best_overlaps(*cols, strand, max_overhang=1000, min_ratio_permille=800, skip=skip)
    read_len = cols[0].cpu().numpy()
    tables = [("stream", best["partner"], best["span"], best["flags"])]
    tables.append(("chains",) + chains_table(np.random.default_rng(5), read_len, args.chain))
    del cols[1:], strand
    torch.cuda.empty_cache()
    out = {"n_reads": n_reads, "n_rec": n_rec, "device": torch.cuda.get_device_name(0), "rounds": 0, "tables": []}
    for name, partner, span, flags in tables:
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (partner, span, flags)]
        t, got = [], None
        for i in range(args.warm + args.calls):
            got = eng.unitigs(cols[0], *d)
            if i >= args.warm:
                t.append(got["kernel_seconds"])
        with tempfile.NamedTemporaryFile(suffix=".utg") as f:
            f.write(np.int32(n_reads).tobytes())
            for x in (read_len, partner, span, flags):
                f.write(np.ascontiguousarray(x).tobytes())
            f.flush()
            w = subprocess.run([WALK, f.name, "3"], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
        s = got["summary"]
        assert w[0] == "WALK" and [int(x) for x in w[1:9]] == [n_reads, s["unitigs"], s["singletons"], s["circular"], s["longest_reads"],
                                                             s["longest_length"], s["total_length"], s["reads_skipped"]], (w, s)
        out["tables"].append({"name": name, "device": t, "walk": [float(x) for x in w[9:]], "launches": got["launches"], "summary": s,
                              "mutual_ends": int(((flags & 2) != 0).sum() + ((flags & 8) != 0).sum())})
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="0 = the bench's default size")
    ap.add_argument("--chain", type=int, default=1000, help="reads per chain of the table made directly")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitigs_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-limit", type=int, default=420, help="seconds the process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    build_walk()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reads", str(args.reads), "--chain", str(args.chain), "--calls", str(args.calls),
           "--warm", str(args.warm)]
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
    n = res["n_reads"]
    rounds = 0
    while (1 << rounds) < 2 * n:
        rounds += 1
    say("one session on one device: figures of a single run, not a distribution over machines or days")
    say(f"set: bench.py workload hg002, {n} reads, {res['n_rec']} records; device {res['device']}")
    say(f"method: one process; per table {args.calls} calls of raft_hip_unitigs_device after {args.warm} warm ones, HIP events on the context's stream; "
        f"the yardstick tools/unitig_walk.cpp (g++ -O2, one host thread) on the same arrays, three repeats; rounds per ranking = {rounds}")
    for t in res["tables"]:
        md, mw = statistics.median(t["device"]), statistics.median(t["walk"])
        cycle_pass = t["launches"] > 1 + rounds + 4
        say(f"table {t['name']}: mutual ends = {t['mutual_ends']}  ({', '.join(f'{k} = {v}' for k, v in t['summary'].items())})")
        say(f"  raft_hip_unitigs_device   median {md * 1e3:9.3f} ms  (min {min(t['device']) * 1e3:.3f}, max {max(t['device']) * 1e3:.3f}; n = {len(t['device'])})  "
            f"launches = {t['launches']}, the cycle pass {'ran' if cycle_pass else 'did not run'}")
        say(f"  sequential walk, one core median {mw * 1e3:9.3f} ms  (min {min(t['walk']) * 1e3:.3f}, max {max(t['walk']) * 1e3:.3f}; n = {len(t['walk'])})  "
            f"walk time / device time = {mw / md:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
