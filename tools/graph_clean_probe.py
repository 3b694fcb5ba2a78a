#!/usr/bin/env python3
"""Device time of raft_hip_graph_clean_device on the string graph of the bench's set, beside raft_hip_string_graph_device and
raft_hip_unitigs_device in the same process (GPU box).

  python tools/graph_clean_probe.py [--reads N] [--out profiles/graph_clean_timing.txt]

One process: the set resident in HBM, overlap_ends for the mask of contained reads, string_graph for the edge list, then
kernel_seconds of graph_clean -- HIP events on the context's stream around its launches, the waits between them not counted -- as the
median of ``--calls`` calls after ``--warm`` warm ones, under miniasm's parameters (W = 500, T = 4, R = 3), and the unitigs of the
table before and after."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, F, Z = 1000, 800, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
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
    cols = [eng.device_copy(t.contiguous()) for t in (o.read_len,) + tuple(o.columns())]
    strand = eng.device_copy((torch.rand(o.n_rec, device=dev, generator=gen) < 0.5).to(torch.uint8))
    n_rec = int(o.n_rec)
    del o
    torch.cuda.empty_cache()
    eng.use_torch_stream()
    ends = eng.overlap_ends(*cols, strand, max_overhang=H, min_ratio_permille=F, symmetric=True)
    skip_host = (np.asarray(ends["status"]) == engine.END_READ_CONTAINED).astype(np.uint8)
    skip = eng.device_copy(torch.from_numpy(skip_host).to(dev))
    g = eng.string_graph(*cols, strand, max_overhang=H, min_ratio_permille=F, fuzz=Z, symmetric=True, skip=skip)
    edges = [eng.device_copy(torch.from_numpy(g[k]).to(dev)) for k in ("edge_u", "edge_w", "edge_span")]
    secs, wall, c = [], [], None
    for i in range(args.warm + args.calls):
        t0 = time.perf_counter()
        c = eng.graph_clean(cols[0], *edges, skip=skip)
        if i >= args.warm:
            secs.append(c["kernel_seconds"])
            wall.append(time.perf_counter() - t0)
    L = cols[0].cpu().numpy()
    before = eng.unitigs(L, g["partner"], g["span"], g["flags"])
    after = eng.unitigs(L, c["partner"], c["span"], c["flags"])

    def n50(lengths):
        v = np.sort(np.asarray(lengths, np.int64))[::-1]
        return int(v[np.searchsorted(np.cumsum(v) * 2, v.sum())]) if v.size else 0
    s = c["summary"]
    text = "\n".join([
        f"graph_clean on the string graph of the bench's hg002 set: {n_reads} reads, {n_rec} records, {s['reads_flagged']} reads flagged as contained, "
        f"{s['edges']} edges; device form, W = 500, T = 4, R = 3; median of {args.calls} calls after {args.warm} warm",
        f"kernel_seconds   {statistics.median(secs) * 1e3:.3f} ms ({min(secs) * 1e3:.3f} .. {max(secs) * 1e3:.3f}), {c['launches']} launches, "
        f"rounds = {s['rounds_run']}, converged = {s['converged']}",
        f"whole call       {statistics.median(wall) * 1e3:.3f} ms on the host's clock (the waits, the copies out and the allocation of the results included)",
        f"string_graph     {g['kernel_seconds'] * 1e3:.3f} ms, {g['launches']} launches (one call, same process)",
        f"summary          {s}",
        f"unitigs before   {before['summary']['unitigs']} unitigs, N50 = {n50(before['utg_length'])}",
        f"unitigs after    {after['summary']['unitigs']} unitigs, N50 = {n50(after['utg_length'])}",
    ]) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
