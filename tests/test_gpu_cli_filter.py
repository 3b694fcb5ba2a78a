"""GPU: `raft --min-identity PCT --min-overlap BASES` -- the records that pass go into the job, and the job is the job on a file of the
kept lines.  On tests/golden/filter/ (made by tests/golden/make_filter_golden.py with the compiled reference on PAF text filtered in
Python) the four files and stdout are the reference's, byte for byte, plus the option's one line; on a synthetic set of 2000 reads
the job with the options equals the job without them on the pre-filtered text -- alone, with --read-stats, with -e auto and on two
contexts."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
from raft_testlib import GOLDEN, ROOT, md5, write_fasta

pytestmark = pytest.mark.gpu
RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")
FILES = ("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed")
FIX = os.path.join(GOLDEN, "filter")
FIXTURE = json.load(open(os.path.join(FIX, "fixture.json")))
LINE = "INFO, filter_overlaps(), "
CMD = "INFO, main(), CMD:"


def run(cwd, args, **env):
    r = subprocess.run([RAFT] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, **env))
    return r.returncode, r.stdout.decode()


def strip_timing(out):
    return "\n".join(l for l in out.split("\n") if not l.startswith("INFO, main(), program completed after") and not l.startswith(CMD))


def options(P, L):
    """The two options as a user writes them: per cent with at most one decimal digit."""
    pct = f"{P // 10}.{P % 10}" if P % 10 else str(P // 10)
    return (["--min-identity", pct] if P else []) + (["--min-overlap", str(L)] if L else [])


def keeps(line, P, L):
    """The rule of include/raft_hip_flt.h on one PAF line of ten fields or more."""
    f = line.split("\t")
    qs, qe, ts, te, matches = int(f[2]), int(f[3]), int(f[7]), int(f[8]), int(f[9])
    block = int(f[10]) if len(f) >= 11 else 0
    return (P == 0 or (block > 0 and matches >= 0 and matches * 1000 >= P * block)) and (L == 0 or (qe - qs >= L and te - ts >= L))


def the_line(P, L, lines):
    return (f"{LINE}min_identity = {P} per mille, min_overlap = {L}, records = {len(lines)}, kept = {sum(keeps(l, P, L) for l in lines)}, "
            f"below identity = {sum(not keeps(l, P, 0) for l in lines)}, below overlap = {sum(not keeps(l, 0, L) for l in lines)}")


def split_out(out, want_line):
    """The option's line stands directly behind the reference's own last line (CMD); -> stdout without it and without the timing lines."""
    lines = out.split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith(LINE)]
    assert len(at) == 1 and lines[at[0] - 1].startswith(CMD) and lines[at[0]] == want_line, (lines[-6:], want_line)
    return strip_timing("\n".join(lines[:at[0]] + lines[at[0] + 1:]))


@pytest.mark.parametrize("setting", FIXTURE["settings"], ids=lambda s: f"P{s['min_identity_permille']}_L{s['min_overlap']}")
def test_the_fixture_of_the_reference(tmp_path, setting):
    P, L = setting["min_identity_permille"], setting["min_overlap"]
    write_fasta(tmp_path / "reads.fa", FIXTURE["names"], FIXTURE["lengths"])
    text = open(os.path.join(FIX, "overlaps.paf")).read()
    (tmp_path / "overlaps.paf").write_text(text)
    lines = text.split("\n")[:-1]
    assert len(lines) == FIXTURE["n_records"] and sum(keeps(l, P, L) for l in lines) == setting["kept"]
    rc, out = run(tmp_path, FIXTURE["args"] + options(P, L) + ["reads.fa", "overlaps.paf"])
    assert rc == 0, out
    want_line = (f"{LINE}min_identity = {P} per mille, min_overlap = {L}, records = {FIXTURE['n_records']}, kept = {setting['kept']}, "
                 f"below identity = {setting['below_identity']}, below overlap = {setting['below_overlap']}")
    assert want_line == the_line(P, L, lines)
    assert split_out(out, want_line) == setting["stdout"]
    assert f"INFO, Symmetric overlaps {setting['symmetric']} \n" in out
    for f in FILES:
        got = open(tmp_path / ("out." + f), "rb").read()
        assert md5(got) == setting["md5"][f], f
        if f != "reads.fasta":
            assert got == open(os.path.join(FIX, f"p{P}_l{L}", "expect.out." + f), "rb").read(), f


def test_without_the_options_nothing_changes(tmp_path):
    """... and a setting that drops nothing gives the unfiltered job and says so."""
    write_fasta(tmp_path / "reads.fa", FIXTURE["names"], FIXTURE["lengths"])
    text = open(os.path.join(FIX, "overlaps.paf")).read()
    (tmp_path / "overlaps.paf").write_text(text)
    rc, plain = run(tmp_path, FIXTURE["args"][:-1] + ["plain", "reads.fa", "overlaps.paf"])
    assert rc == 0 and LINE not in plain, plain
    rc, out = run(tmp_path, FIXTURE["args"][:-1] + ["all", "--min-overlap", "1", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    n = FIXTURE["n_records"]
    assert split_out(out, f"{LINE}min_identity = 0 per mille, min_overlap = 1, records = {n}, kept = {n}, below identity = 0, below overlap = 0") == strip_timing(plain)
    for f in FILES:
        assert open(tmp_path / ("all." + f), "rb").read() == open(tmp_path / ("plain." + f), "rb").read(), f


@pytest.mark.parametrize("bad", [["--min-identity", "0"], ["--min-identity", "100.1"], ["--min-identity", "99.55"], ["--min-identity", "1e2"],
                                 ["--min-identity", ""], ["--min-overlap", "0"], ["--min-overlap", "-5"], ["--min-overlap", "2147483648"],
                                 ["--min-overlap", "1k"]], ids=lambda b: " ".join(b))
def test_a_bad_value_is_the_usage_error(tmp_path, bad):
    rc, out = run(tmp_path, ["-e", "3"] + bad + ["reads.fa", "overlaps.paf"])
    assert rc == 1 and out.startswith("Usage: raft [options] <input-reads.fa> <in.paf>\n"), out
    assert os.listdir(tmp_path) == []


P_SYN, L_SYN = 985, 2000


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """2000 reads, a symmetric PAF with identities of 960 to 1000 per mille by pair of reads, some ten-field lines; beside it the text
    that holds exactly the lines (985 per mille, 2000 bases) keeps."""
    from raft_amd.synth import make_overlaps
    d = tmp_path_factory.mktemp("flt_cli")
    o = make_overlaps(2000, coverage=30, seed=5)
    rl = o.read_len.numpy()
    qid, qs, qe, tid, ts, te = (c.numpy().astype(np.int64) for c in o.columns())
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(d / "reads.fa", names, rl)
    block = np.maximum(qe - qs, te - ts) + 3
    pm = 960 + ((np.minimum(qid, tid) * 2 ** 20 + np.maximum(qid, tid)) * 7919 + 13) % 41
    matches = -(-block * pm // 1000)
    lines = []
    for i in range(qid.size):
        f = [names[qid[i]], str(rl[qid[i]]), str(qs[i]), str(qe[i]), "+", names[tid[i]], str(rl[tid[i]]), str(ts[i]), str(te[i]), str(matches[i]), str(block[i]), "60"]
        lines.append("\t".join(f[:10] if i % 1009 == 7 else f))
    kept = [l for l in lines if keeps(l, P_SYN, L_SYN)]
    assert 0.2 * len(lines) < len(kept) < 0.8 * len(lines)
    (d / "overlaps.paf").write_text("".join(l + "\n" for l in lines))
    (d / "kept.paf").write_text("".join(l + "\n" for l in kept))
    return d, lines


@pytest.mark.parametrize("extra,env,est", [([], {}, "20"), (["--read-stats"], {}, "20"), ([], {}, "auto"), ([], {"RAFT_DEVICES": "0,0"}, "20"),
                                           ([], {"RAFT_RANKS": "2"}, "20")],
                         ids=["alone", "read_stats", "auto", "two_contexts", "two_ranks"])
def test_the_job_on_the_pre_filtered_text(synthetic, extra, env, est):
    d, lines = synthetic
    tag = re.sub(r"\W", "", "_".join(extra + list(env) + [est]))
    rc, want = run(d, ["-e", est] + extra + ["-o", "w" + tag, "reads.fa", "kept.paf"], **env)
    assert rc == 0, want
    rc, got = run(d, ["-e", est] + extra + options(P_SYN, L_SYN) + ["-o", "g" + tag, "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, got
    assert split_out(got, the_line(P_SYN, L_SYN, lines)) == strip_timing(want)
    made = sorted(f[len("w" + tag) + 1:] for f in os.listdir(d) if f.startswith("w" + tag + "."))
    assert set(FILES) <= set(made) and (not extra or "read_stats.tsv" in made)
    for f in made:
        assert md5(open(d / f"g{tag}.{f}", "rb").read()) == md5(open(d / f"w{tag}.{f}", "rb").read()), f
    assert f"length of alignments  {sum(keeps(l, P_SYN, L_SYN) for l in lines)}()" in got
