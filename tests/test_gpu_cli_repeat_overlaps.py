"""GPU: `raft --repeat-overlaps A` -- PREFIX.repeat_overlaps.tsv and PREFIX.repeat_overlaps.records.tsv (raft_hip_repeat_overlaps_host on the
tokenised columns and the job's own repeat arrays).  Both tables equal text rendered from the model (tests/test_repeat_overlaps_cases.py
want_classes) on the job's own outputs -- the PAF as read back, the runs of the job's long_repeats.txt, the flag of its stdout --; the
reference's four files and every earlier stdout line are byte for byte those of the run without the option; the new line is last."""
import os
import subprocess

import numpy as np
import pytest
from raft_testlib import parse_long_repeats, write_fasta, write_paf
from test_gpu_cli_read_stats import FILES, RAFT, read_fasta, read_paf, read_tsv, strip_timing
from test_repeat_overlaps_cases import csr, golden_case, want_classes
from test_repeat_overlaps_writer import restate_reads, restate_records

pytestmark = pytest.mark.gpu
LINE = "INFO, repeat_overlaps(), "
NEW = ("repeat_overlaps.tsv", "repeat_overlaps.records.tsv")


def run(cwd, args, **env):
    r = subprocess.run([RAFT] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, **env))
    return r.returncode, r.stdout.decode()


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """A symmetric PAF of 142,348 records over 1500 reads; under -e 20 it has 822 repeats, up to four on a read, and 1396 contained reads."""
    from raft_amd.synth import make_overlaps
    d = tmp_path_factory.mktemp("ovl_cli")
    o = make_overlaps(1500, coverage=30, seed=3)
    cols = [c.numpy() for c in (o.read_len,) + o.columns()]
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(d / "reads.fa", names, cols[0])
    write_paf(d / "overlaps.paf", names, *cols)
    return d


def with_and_without(d, options, anchor, extra=(), env={}):
    """Runs `raft options -o b` and `raft options --repeat-overlaps anchor extra -o a` in d; checks what must not change; returns the model
    on the job's own outputs and the tables' text."""
    rc, out_b = run(d, options + ["-o", "b", "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, out_b
    rc, out_a = run(d, options + ["--repeat-overlaps", str(anchor)] + list(extra) + ["-o", "a", "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, out_a
    before = sorted(f[2:] for f in os.listdir(d) if f.startswith("b."))
    assert sorted(f[2:] for f in os.listdir(d) if f.startswith("a.")) == sorted(before + list(NEW))
    assert set(FILES) <= set(before)
    for f in before:
        assert open(d / ("a." + f), "rb").read() == open(d / ("b." + f), "rb").read(), f
    lines_a, lines_b = strip_timing(out_a).split("\n"), strip_timing(out_b).split("\n")
    assert lines_a[-1] == "" and lines_a[-2].startswith(LINE) and lines_a[:-2] + [""] == lines_b
    assert not any(LINE in l for l in lines_b)
    # the model on the job's own outputs
    names, length = read_fasta(d / "reads.fa")
    cols = read_paf(d / "overlaps.paf", names)
    symmetric = int([l for l in lines_a if l.startswith("INFO, Symmetric overlaps")][0].split()[3])
    rep = csr(parse_long_repeats(open(d / "a.long_repeats.txt").read()))
    w = want_classes(length, *cols, bool(symmetric), anchor, *rep)
    assert open(d / "a.repeat_overlaps.tsv").read() == restate_reads(names, length, w["read_touch"], w["read_repeat"], w["read_flags"])
    assert open(d / "a.repeat_overlaps.records.tsv").read() == restate_records(names, *cols, w["cls"])
    assert lines_a[-2] == (f"{LINE}min_anchor = {anchor}, records = {w['n_records']}, query side in a repeat = {w['q_repeat']}, target side = "
                           f"{w['t_repeat']}, both = {w['both_repeat']}, contained reads = {w['reads_contained']}, contained only inside repeats = "
                           f"{w['reads_repeat_contained']}")
    return w, lines_a


def test_with_read_stats_and_low_cov(synthetic):
    w, lines = with_and_without(synthetic, ["-e", "20", "--read-stats", "--low-cov", "0"], 1000)
    assert lines[-4].startswith("INFO, read_stats(), ") and lines[-3].startswith("INFO, low_coverage(), ")
    assert w["q_repeat"] > 0 and w["both_repeat"] > 0 and 0 < w["reads_repeat_contained"] < w["reads_contained"]
    assert 0 < int((w["cls"] & 3 != 0).sum()) < w["n_records"]
    # who is contained: the census's flags of read_stats.tsv and the new table agree
    t = read_tsv(synthetic / "a.read_stats.tsv")
    table = [l.split("\t") for l in open(synthetic / "a.repeat_overlaps.tsv").read().split("\n")[:-1]]
    assert [r[0] for r in table] == t["name"] and [int(r[1]) for r in table] == t["length"]
    assert [r[4] != "no" for r in table] == [c != 0 for c in t["contained"]]
    assert {r[4] for r in table} == {"no", "anchored", "repeat"}


def test_under_auto(synthetic):
    w, lines = with_and_without(synthetic, ["-e", "auto"], 500)
    assert any(l.startswith("INFO, estimate_coverage(), est_cov = ") for l in lines) and w["q_repeat"] > 0


def test_on_two_contexts(synthetic):
    w, _ = with_and_without(synthetic, ["-e", "20"], 1000, env={"RAFT_DEVICES": "0,0"})
    assert w["q_repeat"] > 0 and w["reads_repeat_contained"] > 0


def test_with_the_input_prepared_by_the_cli(synthetic):
    """RAFT_CLI_PREPARE=1 writes window records over the tokenised query column before the job: the option reads the ids it kept."""
    w, _ = with_and_without(synthetic, ["-e", "20"], 1000, env={"RAFT_CLI_PREPARE": "1"})
    assert w["q_repeat"] > 0


def test_a_stream_that_is_not_symmetric(tmp_path):
    cols, _ = golden_case("s300_nonsym_shuffled")
    names = [f"read{i}" for i in range(cols[0].size)]
    write_fasta(tmp_path / "reads.fa", names, cols[0])
    write_paf(tmp_path / "overlaps.paf", names, *cols)
    w, lines = with_and_without(tmp_path, ["-e", "15"], 2000)
    assert "INFO, Symmetric overlaps 0 " in lines
    assert w["q_repeat"] > 0 and w["t_repeat"] > 0 and (w["cls"] & 3 == 2).any()
