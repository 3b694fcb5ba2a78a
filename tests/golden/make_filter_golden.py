#!/usr/bin/env python3
"""Generates tests/golden/filter/ by RUNNING THE COMPILED REFERENCE on PAF text filtered here, in Python.

Only works in the build container (needs oracle/_ref/raft, built by `make -C oracle`).  The fixture is data: a PAF with varied columns
10 and 11 (and some ten-field lines) over 40 reads, and for each of three settings of `raft --min-identity / --min-overlap` what the
unmodified reference writes for the file that holds exactly the kept lines -- the rule of include/raft_hip_flt.h restated on the
text.  No reference source is stored.

  filter/overlaps.paf            the unfiltered input
  filter/fixture.json            the reads (names, lengths: the bases are raft_testlib.seq_of's), the reference's arguments, and per
                                 setting P, L, the counts, the reference's stdout and the md5 of its four files
  filter/p<P>_l<L>/expect.*      the reference's coverage.txt, long_repeats.txt and long_repeats.bed (reads.fasta: by md5 only, it is
                                 as large as the reads)

The recipe refuses to write unless the inputs are worth testing on: every setting drops at least a fifth and keeps at least a fifth
of the records; every kept stream still yields a repeat and a read cut into two or more fragments; the (995, 300) stream differs from
the unfiltered one in its symmetric flag or in its first record.

Usage:  python tests/golden/make_filter_golden.py
"""
from __future__ import annotations

import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from raft_testlib import REF_BIN, md5, run_ref_binary, write_fasta  # noqa: E402

OUT_FILES = ("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed")
KEPT_AS_TEXT = OUT_FILES[1:]
SETTINGS = ((990, 0), (0, 500), (995, 300))
ARGS = ["-r", "50", "-e", "3", "-m", "1.5", "-l", "600", "-p", "300", "-f", "100", "-v", "50", "-o", "out"]
N_READS = 40


def strip_timing(stdout: bytes) -> str:
    return "\n".join(ln for ln in stdout.decode().split("\n")
                     if not ln.startswith("INFO, main(), program completed after") and not ln.startswith("INFO, main(), CMD:"))


def keeps(line: str, P: int, L: int) -> bool:
    """The rule on one PAF line of ten fields or more (block = 0 on a ten-field line)."""
    f = line.split("\t")
    qs, qe, ts, te, matches = int(f[2]), int(f[3]), int(f[7]), int(f[8]), int(f[9])
    block = int(f[10]) if len(f) >= 11 else 0
    identity_ok = P == 0 or (block > 0 and matches >= 0 and matches * 1000 >= P * block)
    span_ok = L == 0 or (qe - qs >= L and te - ts >= L)
    return identity_ok and span_ok


def make_inputs(seed: int = 7):
    """Reads laid on a line of 9 kb, every pair that shares 120 bases or more as two mirrored records grouped by query; one repeat of
    700 bases carried by 12 reads, each pair of which overlaps on it.  Identity per pair of reads, 975 to 1000 per mille."""
    rng = np.random.default_rng(seed)
    length = rng.integers(800, 1500, N_READS)
    start = np.sort(rng.integers(0, 9000, N_READS))
    names = [f"flt{i:02d}" for i in range(N_READS)]
    carriers = np.sort(rng.choice(N_READS, 12, replace=False))
    rep_at = {int(r): int(rng.integers(0, length[r] - 700)) for r in carriers}
    permille = {}
    pairs = []                                            # (query, qs, qe, target, ts, te)
    for a in range(N_READS):
        for b in range(N_READS):
            if a == b:
                continue
            lo, hi = max(start[a], start[b]), min(start[a] + length[a], start[b] + length[b])
            if hi - lo >= 120:
                pairs.append((a, lo - start[a], hi - start[a], b, lo - start[b], hi - start[b]))
            if a in rep_at and b in rep_at:
                pairs.append((a, rep_at[a], rep_at[a] + 700, b, rep_at[b], rep_at[b] + 700))
    pairs.sort(key=lambda r: r[0])
    lines = []
    for i, (a, qs, qe, b, ts, te) in enumerate(pairs):
        key = (min(a, b), max(a, b), qe - qs)
        if key not in permille:
            permille[key] = int(rng.integers(975, 1001))
        block = max(qe - qs, te - ts) + 5
        matches = -(-block * permille[key] // 1000)
        f = [names[a], str(length[a]), str(qs), str(qe), "+", names[b], str(length[b]), str(ts), str(te), str(matches), str(block), "60", "tp:A:P"]
        n_fields = 10 if i % 37 == 20 else (11 if i % 5 == 0 else (12 if i % 5 == 1 else 13))
        lines.append("\t".join(f[:n_fields]))
    return names, length, lines


def first_record_and_flag(lines):
    """The first record's six values and the symmetric flag (chop.hpp:171-184) of a PAF given as lines."""
    rec = [(f[0], int(f[2]), int(f[3]), f[5], int(f[7]), int(f[8])) for f in (ln.split("\t") for ln in lines)]
    if not rec:
        return None, 0
    q, qs, qe, t, ts, te = rec[0]
    return rec[0], int(any(r == (t, ts, te, q, qs, qe) for r in rec[1:]))


def main():
    assert os.path.exists(REF_BIN), "oracle/_ref/raft missing: run `make -C oracle` in the build container"
    names, length, lines = make_inputs()
    root = os.path.join(HERE, "filter")
    fixture = {"names": names, "lengths": [int(x) for x in length], "args": ARGS, "n_records": len(lines), "settings": []}
    unfiltered = first_record_and_flag(lines)
    staged = {}
    assert 200 <= len(lines) <= 900 and sum(ln.count("\t") == 9 for ln in lines) >= 3, len(lines)
    for P, L in SETTINGS:
        kept = [ln for ln in lines if keeps(ln, P, L)]
        assert 5 * len(kept) >= len(lines) and 5 * (len(lines) - len(kept)) >= len(lines), (P, L, len(kept), len(lines))
        below_identity = sum(not keeps(ln, P, 0) for ln in lines)
        below_span = sum(not keeps(ln, 0, L) for ln in lines)
        with tempfile.TemporaryDirectory() as tmp:
            write_fasta(os.path.join(tmp, "reads.fa"), names, length)
            with open(os.path.join(tmp, "overlaps.paf"), "w") as f:
                f.write("".join(ln + "\n" for ln in kept))
            rc, out = run_ref_binary(tmp, ARGS, "reads.fa", "overlaps.paf")
            assert rc == 0, out.decode()
            files = {name: open(os.path.join(tmp, "out." + name), "rb").read() for name in OUT_FILES}
        n_repeats = sum(ln.count(",") - 1 for ln in files["long_repeats.txt"].decode().split("\n") if ln)
        headers = [ln for ln in files["reads.fasta"].decode().split("\n") if ln.startswith(">")]
        per_read = {}
        for h in headers:
            per_read[h.split(",")[1]] = per_read.get(h.split(",")[1], 0) + 1
        assert n_repeats >= 1 and max(per_read.values()) >= 2, (P, L, n_repeats, max(per_read.values()))
        first, flag = first_record_and_flag(kept)
        if (P, L) == (995, 300):
            assert (first, flag) != unfiltered and (first != unfiltered[0] or flag != unfiltered[1]), (first, flag, unfiltered)
        fixture["settings"].append({"min_identity_permille": P, "min_overlap": L, "kept": len(kept), "below_identity": below_identity,
                                    "below_overlap": below_span, "symmetric": flag, "first_kept": lines.index(kept[0]), "n_repeats": n_repeats,
                                    "n_fragments": len(headers), "stdout": strip_timing(out), "md5": {k: md5(v) for k, v in files.items()}})
        staged[f"p{P}_l{L}"] = {k: files[k] for k in KEPT_AS_TEXT}
    # every condition holds: write
    if os.path.isdir(root):
        shutil.rmtree(root)
    os.makedirs(root)
    with open(os.path.join(root, "overlaps.paf"), "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    for d, files in staged.items():
        os.makedirs(os.path.join(root, d))
        for k, v in files.items():
            with open(os.path.join(root, d, "expect.out." + k), "wb") as f:
                f.write(v)
    with open(os.path.join(root, "fixture.json"), "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(dp, fn)) for dp, _, fns in os.walk(root) for fn in fns)
    print(f"{len(lines)} records, unfiltered first record {unfiltered[0]} flag {unfiltered[1]}; {total} bytes in {root}")
    for s in fixture["settings"]:
        print({k: v for k, v in s.items() if k not in ("stdout", "md5")})


if __name__ == "__main__":
    main()
