#!/usr/bin/env python3
"""Tail sets through the compiled reference binary: tests/golden/tail_ref.npz.

Build container only (needs oracle/_ref/raft, built by `make -C oracle`).  raft_testlib.tail_ref_list() names the cases: tail_markers
under every (div, overlap, flank) and a thinned tail_counts, regenerated with repeat_length = interval_length = L (the command line
sets both with -p) and runs of at least L bases.  Every case is written as FASTA + PAF text and run through the unmodified `raft`
binary, whose result files are parsed back into integer arrays (as make_ref_fuzz.py does).

The fixture is data only: the inputs once per (set, div, flank) -- read lengths and the query columns; all records are self
overlaps, the target columns repeat them -- with the coverage the binary printed for them, and per parameter triple the parsed
repeats and fragments, the stdout statistics and the md5 of the four result files.

Usage:  python tests/golden/make_tail_ref.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from raft_testlib import (REF_BIN, md5, result_from_ref_files, run_ref_binary, tail_ref_build, tail_ref_list, write_fasta,  # noqa: E402
                          write_paf)

OUT_FILES = ("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed")


def main():
    assert os.path.exists(REF_BIN), "oracle/_ref/raft missing: run `make -C oracle` in the build container"
    inputs, input_of = {}, []
    cat_in = {k: [] for k in ("read_len", "qid", "qs", "qe", "cov")}
    cat_out = {k: [] for k in ("rep_cnt", "rep_s", "rep_e", "frag_read", "frag_begin", "frag_end")}
    offs = {k: [0] for k in ("reads", "recs", "cov", "reads_out", "rep", "frag")}
    P, sym, stats, md = [], [], [], []
    for (name, div, overlap, flank) in tail_ref_list():
        case = tail_ref_build(name, div, overlap, flank)
        p, cols = case.p, case.cols
        cli = type(p)(**dict(p.__dict__, symmetric_mode=-1))
        names = [f"r{i}" for i in range(len(cols[0]))]
        with tempfile.TemporaryDirectory() as tmp:
            write_fasta(os.path.join(tmp, "reads.fa"), names, cols[0])
            write_paf(os.path.join(tmp, "overlaps.paf"), names, *cols)
            rc, out = run_ref_binary(tmp, cli.cli_args() + ["-o", "out"], "reads.fa", "overlaps.paf")
            assert rc == 0, (name, div, overlap, flank, rc, out[-300:])
            res = result_from_ref_files(os.path.join(tmp, "out"), names)
            md.append([md5(open(os.path.join(tmp, "out." + f), "rb").read()) for f in OUT_FILES])
        text = out.decode()
        sym.append(int("INFO, Symmetric overlaps 1 " in text))
        stats.append("\n".join(l for l in text.split("\n") if l.startswith(("coverage per window", "fraction_of_repeat_length"))))
        P.append([p.reso, p.est_cov, p.repeat_length, p.interval_length, p.read_length, p.overlap_length, p.flanking_length])
        key = (name, div, flank)
        assert res["cov"].max(initial=0) <= 255
        if key not in inputs:
            inputs[key] = (len(inputs), res["cov"])
            for k, a in zip(("read_len", "qid", "qs", "qe"), cols[:4]):
                cat_in[k].append(np.asarray(a, np.int32))
            cat_in["cov"].append(res["cov"].astype(np.uint8))
            offs["reads"].append(offs["reads"][-1] + len(cols[0]))
            offs["recs"].append(offs["recs"][-1] + len(cols[1]))
            offs["cov"].append(offs["cov"][-1] + len(res["cov"]))
        assert np.array_equal(inputs[key][1], res["cov"])           # (the overlap changes no input and no coverage)
        input_of.append(inputs[key][0])
        cat_out["rep_cnt"].append(np.diff(res["rep_offset"]).astype(np.int32))
        for k in ("rep_s", "rep_e", "frag_read", "frag_begin", "frag_end"):
            cat_out[k].append(res[k])
        offs["reads_out"].append(offs["reads_out"][-1] + len(cols[0]))
        offs["rep"].append(offs["rep"][-1] + len(res["rep_s"]))
        offs["frag"].append(offs["frag"][-1] + len(res["frag_read"]))
    arrays = {k: np.concatenate(v).astype(np.uint8 if k == "cov" else np.int32) for k, v in {**cat_in, **cat_out}.items()}
    path = os.path.join(HERE, "tail_ref.npz")
    np.savez_compressed(path, triples=np.array([t[1:] for t in tail_ref_list()], np.int32), params=np.array(P, np.int32),
                        input_of=np.array(input_of, np.int32), symmetric=np.array(sym, np.int32), stats=np.array(stats), md5=np.array(md),
                        **{"off_" + k: np.array(v, np.int64) for k, v in offs.items()}, **arrays)
    print(f"tail_ref.npz: {len(P)} cases over {len(inputs)} inputs, {offs['reads'][-1]} reads, {offs['recs'][-1]} records, {offs['cov'][-1]} windows, "
          f"{offs['rep'][-1]} repeats, {offs['frag'][-1]} fragments, symmetric {sorted(set(sym))}, {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
