"""GPU: `raft --fragment-overlaps` -- PREFIX.fragments.tsv (raft_hip_frag_overlaps_host on the tokenised columns and the job's own fragment
rows and repeat arrays).  The table equals text rendered from the model (tests/test_fragment_overlaps_cases.py want_fragments) on the
job's own outputs -- the PAF as read back, the fragments of the headers of its reads.fasta, the runs of its long_repeats.txt, the flag of
its stdout --; the reference's four files and every earlier stdout line are byte for byte those of the run without the option; the new
line is last."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from raft_testlib import GOLDEN, parse_fasta_headers, parse_long_repeats, write_fasta, write_paf
from test_fragment_overlaps_cases import classes, want_fragments
from test_fragment_overlaps_writer import restate
from test_gpu_cli_read_stats import FILES, RAFT, read_fasta, read_paf, strip_timing
from test_repeat_overlaps_cases import csr

pytestmark = pytest.mark.gpu
LINE = "INFO, fragment_overlaps(), "
NEW = "fragments.tsv"
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))
MICRO = ("g1", "g2", "g4", "g6_mirrored_pair", "g7_half_pair")          # (real reads written under the default prefix: headers that name read and position)


def run(cwd, args, **env):
    r = subprocess.run([RAFT] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, **env))
    return r.returncode, r.stdout.decode()


def with_and_without(d, options, extra=(), env={}, reads="reads.fa"):
    """Runs `raft options -o b` and `raft options --fragment-overlaps extra -o a` in d; checks what must not change; returns the model on
    the job's own outputs and the stdout lines."""
    rc, out_b = run(d, options + ["-o", "b", reads, "overlaps.paf"], **env)
    assert rc == 0, out_b
    rc, out_a = run(d, options + ["--fragment-overlaps"] + list(extra) + ["-o", "a", reads, "overlaps.paf"], **env)
    assert rc == 0, out_a
    before = sorted(f[2:] for f in os.listdir(d) if f.startswith("b."))
    new = sorted(set(f[2:] for f in os.listdir(d) if f.startswith("a.")) - set(before))
    assert NEW in new and set(FILES) <= set(before)
    for f in before:
        assert open(d / ("a." + f), "rb").read() == open(d / ("b." + f), "rb").read(), f
    lines_a, lines_b = strip_timing(out_a).split("\n"), strip_timing(out_b).split("\n")
    assert lines_a[-1] == "" and lines_a[-2].startswith(LINE) and not any(LINE in l for l in lines_b)
    earlier = [l for l in lines_a[:-2] if not any(l.startswith(f"INFO, {o}(), ") for o in ("read_stats", "low_coverage", "repeat_overlaps"))]
    assert earlier + [""] == lines_b
    # the model on the job's own outputs
    names, length = read_fasta(d / reads)
    cols = read_paf(d / "overlaps.paf", names)
    symmetric = int([l for l in lines_a if l.startswith("INFO, Symmetric overlaps")][0].split()[3])
    headers = parse_fasta_headers(open(d / "a.reads.fasta").read())
    assert [h[0] for h in headers] == list(range(1, len(headers) + 1))
    index = {n: i for i, n in enumerate(names)}
    owner = [index[h[1].split()[0]] for h in headers]
    assert owner == sorted(owner)
    rows = [[] for _ in names]
    for h, r in zip(headers, owner):
        rows[r].append((h[2], h[3]))
    table = csr(rows)
    rep = csr(parse_long_repeats(open(d / "a.long_repeats.txt").read()))
    w = want_fragments(length, *cols, bool(symmetric), *table, *rep)
    assert open(d / ("a." + NEW)).read() == restate(names, table[0], table[1], table[2], w["frag_touch"], w["frag_span"], w["frag_contained"], w["frag_repeat"])
    assert lines_a[-2] == (f"{LINE}fragments = {w['n_fragments']}, spanned = {w['frags_spanned']}, contained = {w['frags_contained']}, contained with "
                           f"repeat = {w['frags_contained_repeat']}, reads spanned whole = {w['reads_whole_spanned']}, reads with every fragment "
                           f"contained = {w['reads_all_contained']} of {len(names)}")
    return w, table, lines_a


@pytest.mark.parametrize("name", MICRO)
def test_micro_fixtures(tmp_path, name):
    src = os.path.join(GOLDEN, "micro", name)
    shutil.copy(os.path.join(src, "reads.fa"), tmp_path)
    shutil.copy(os.path.join(src, "overlaps.paf"), tmp_path)
    args = [a for a in MAN["micro"][name]["args"] if a not in ("-o", "raft")]
    w, table, _ = with_and_without(tmp_path, args)
    assert w["n_fragments"] > 0
    for f in FILES:                                             # ... and they are the reference's
        assert open(tmp_path / ("a." + f), "rb").read() == open(os.path.join(src, "expect.raft." + f), "rb").read(), (name, f)


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """A symmetric PAF of 142,348 records over 1500 reads; under -e 20 it has 822 repeats and reads cut into several fragments."""
    from raft_amd.synth import make_overlaps
    d = tmp_path_factory.mktemp("frag_cli")
    o = make_overlaps(1500, coverage=30, seed=3)
    cols = [c.numpy() for c in (o.read_len,) + o.columns()]
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(d / "reads.fa", names, cols[0])
    write_paf(d / "overlaps.paf", names, *cols)
    return d


def test_on_a_synthetic_set(synthetic):
    w, table, _ = with_and_without(synthetic, ["-e", "20"])
    seen = classes(w, table)
    assert seen["contained"] and seen["not contained"] and seen["reads with several rows"] and seen["contained with repeat"], seen
    assert 0 < w["frags_contained"] <= w["frags_spanned"] < w["n_fragments"]


def test_with_every_other_option(synthetic):
    w, _, lines = with_and_without(synthetic, ["-e", "auto"], extra=["--read-stats", "--low-cov", "0", "--repeat-overlaps", "1000"])
    assert any(l.startswith("INFO, estimate_coverage(), est_cov = ") for l in lines)
    assert [l.split("(")[0] for l in lines[-5:-1]] == ["INFO, read_stats", "INFO, low_coverage", "INFO, repeat_overlaps", "INFO, fragment_overlaps"]
    assert w["frags_contained"] > 0


def test_on_two_contexts(synthetic):
    w, _, _ = with_and_without(synthetic, ["-e", "20"], env={"RAFT_DEVICES": "0,0"})
    assert w["frags_contained"] > 0


def test_with_the_input_prepared_by_the_cli(synthetic):
    """RAFT_CLI_PREPARE=1 writes window records over the tokenised query column before the job: the option reads the ids it kept."""
    w, _, _ = with_and_without(synthetic, ["-e", "20"], env={"RAFT_CLI_PREPARE": "1"})
    assert w["frags_contained"] > 0
