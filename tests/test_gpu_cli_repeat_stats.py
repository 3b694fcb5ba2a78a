"""GPU: `raft --repeat-stats` -- PREFIX.long_repeats.stats.tsv (raft_hip_repeat_stats_host behind a one-piece pass under the job's final
parameters).  The table's start / end equal long_repeats.txt line for line and its other columns equal text rendered from the model
(tests/test_repeat_stats_cases.py repeat_stats_model) on the job's own outputs -- the PAF as read back, the windows of its coverage.txt,
the runs of its long_repeats.txt, the flag of its stdout --; the reference's four files and every earlier stdout line are byte for byte
those of the run without the option; the new line's numbers are the file's sums; -e auto gives the table of -e N with the N it prints;
the other options change nothing of it."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from raft_testlib import GOLDEN, md5, parse_coverage_txt, parse_long_repeats, write_fasta, write_paf
from test_gpu_cli_read_stats import FILES, RAFT, read_fasta, read_paf, strip_timing
from test_repeat_stats_cases import csr, repeat_stats_model, where_of
from test_repeat_stats_writer import restate

pytestmark = pytest.mark.gpu
LINE = "INFO, repeat_stats(), "
NEW = "long_repeats.stats.tsv"
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))
MICRO = ("g1", "g2", "g3", "g4")
OTHERS = ("read_stats", "low_coverage", "repeat_overlaps", "fragment_overlaps")


def run(cwd, args, **env):
    r = subprocess.run([RAFT] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, **env))
    return r.returncode, r.stdout.decode()


def option(args, flag, default):
    return type(default)(args[args.index(flag) + 1]) if flag in args else default


def with_and_without(d, options, extra=(), env={}, est_cov=None):
    """Runs `raft options -o b` and `raft options --repeat-stats extra -o a` in d; checks what must not change; returns the model on the
    job's own outputs, the table's text and the stdout lines."""
    rc, out_b = run(d, options + ["-o", "b", "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, out_b
    rc, out_a = run(d, options + ["--repeat-stats"] + list(extra) + ["-o", "a", "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, out_a
    before = sorted(f[2:] for f in os.listdir(d) if f.startswith("b."))
    new = sorted(set(f[2:] for f in os.listdir(d) if f.startswith("a.")) - set(before))
    assert NEW in new and set(FILES) <= set(before)
    for f in before:
        assert md5(open(d / ("a." + f), "rb").read()) == md5(open(d / ("b." + f), "rb").read()), f
    lines_a, lines_b = strip_timing(out_a).split("\n"), strip_timing(out_b).split("\n")
    assert lines_a[-1] == "" and lines_a[-2].startswith(LINE) and not any(LINE in l for l in lines_b)
    earlier = [l for l in lines_a[:-2] if not any(l.startswith(f"INFO, {o}(), ") for o in OTHERS)]
    assert earlier + [""] == lines_b
    # the model on the job's own outputs
    names, length = read_fasta(d / "reads.fa")
    cols = read_paf(d / "overlaps.paf", names)
    symmetric = int([l for l in lines_a if l.startswith("INFO, Symmetric overlaps")][0].split()[3])
    runs = parse_long_repeats(open(d / "a.long_repeats.txt").read())
    rep = csr(runs)
    windows = parse_coverage_txt(open(d / "a.coverage.txt").read())
    cov_offset = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.int64)
    cov = np.concatenate(windows + [np.empty(0, np.int32)]).astype(np.int32)
    if est_cov is None:
        est_cov = option(options, "-e", 0)
    threshold = max(int(est_cov * option(options, "-m", 1.5)), 1)
    w = repeat_stats_model(np.asarray(length, np.int32), *cols, bool(symmetric), *rep, threshold=threshold, cov_offset=cov_offset, cov=cov,
                           reso=option(options, "-r", 50))
    text = open(d / ("a." + NEW)).read()
    rows = [ln.split("\t") for ln in text.splitlines()]
    flat = [(names[r], s, e) for r, rr in enumerate(runs) for s, e in rr]
    assert [(f[0], int(f[1]), int(f[2])) for f in rows] == flat                    # long_repeats.txt, line for line
    assert text == restate(names, rep[0], rep[1], rep[2], w["run_flags"], w["run_windows"], w["run_cov_sum"], w["run_cov_min"], w["run_cov_max"],
                           w["run_high"], w["run_touch"], w["run_span"], w["run_inside"])
    # the line's numbers are the file's sums
    where = [f[3] for f in rows]
    assert where == where_of(w["run_flags"])
    spanned = [int(f[10]) > 0 for f in rows]
    assert lines_a[-2] == (f"{LINE}repeats = {len(rows)}, interior = {where.count('interior')}, spanned = {sum(spanned)}, interior spanned = "
                           f"{sum(s and x == 'interior' for s, x in zip(spanned, where))}, untouched = {sum(int(f[9]) == 0 for f in rows)}, "
                           f"sides inside a repeat = {sum(int(f[11]) for f in rows)}")
    return w, text, lines_a


@pytest.mark.parametrize("name", MICRO)
def test_micro_fixtures(tmp_path, name):
    src = os.path.join(GOLDEN, "micro", name)
    shutil.copy(os.path.join(src, "reads.fa"), tmp_path)
    shutil.copy(os.path.join(src, "overlaps.paf"), tmp_path)
    args = [a for a in MAN["micro"][name]["args"] if a not in ("-o", "raft")]
    w, _, _ = with_and_without(tmp_path, args)
    for f in FILES:                                             # ... and they are the reference's
        assert open(tmp_path / ("a." + f), "rb").read() == open(os.path.join(src, "expect.raft." + f), "rb").read(), (name, f)


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """A symmetric PAF of 142,348 records over 1500 reads; under -e 20 it has 822 repeats."""
    from raft_amd.synth import make_overlaps
    d = tmp_path_factory.mktemp("rst_cli")
    o = make_overlaps(1500, coverage=30, seed=3)
    cols = [c.numpy() for c in (o.read_len,) + o.columns()]
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(d / "reads.fa", names, cols[0])
    write_paf(d / "overlaps.paf", names, *cols)
    return d


def test_on_a_synthetic_set(synthetic):
    w, text, _ = with_and_without(synthetic, ["-e", "20"])
    assert w["n_runs"] > 100 and w["runs_interior"] > 0 and 0 < w["interior_spanned"] < w["runs_interior"] and w["sides_inside"] > 0
    assert (w["run_high"] > 0).all() and (w["run_cov_min"] >= w["run_span"]).all()
    (synthetic / "table.tsv").write_text(text)


@pytest.mark.parametrize("extra,env", [(["--read-stats", "--low-cov", "0", "--fragment-overlaps"], {}), ([], {"RAFT_DEVICES": "0,0"}),
                                       ([], {"RAFT_CLI_PREPARE": "1"})], ids=["other_options", "two_contexts", "cli_prepare"])
def test_the_table_is_the_same(synthetic, extra, env):
    """... when the other options are given along, on two contexts, and with the input prepared by the CLI."""
    _, text, lines = with_and_without(synthetic, ["-e", "20"], extra=extra, env=env)
    if not os.path.exists(synthetic / "table.tsv"):                  # (run on its own)
        (synthetic / "table.tsv").write_text(with_and_without(synthetic, ["-e", "20"])[1])
    assert text == open(synthetic / "table.tsv").read()
    if extra:
        assert [l.split("(")[0] for l in lines[-5:-1]] == ["INFO, read_stats", "INFO, low_coverage", "INFO, fragment_overlaps", "INFO, repeat_stats"]


def test_auto_gives_the_table_of_the_number_it_prints(synthetic):
    rc, out = run(synthetic, ["-e", "auto", "--repeat-stats", "-o", "auto", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    est = [l for l in out.split("\n") if l.startswith("INFO, estimate_coverage(), est_cov = ")]
    assert len(est) == 1
    n = int(est[0].split()[-1])
    w, text, lines = with_and_without(synthetic, ["-e", str(n)])
    assert open(synthetic / ("auto." + NEW)).read() == text and w["n_runs"] > 0
    assert [l for l in out.split("\n") if l.startswith(LINE)] == [l for l in lines if l.startswith(LINE)]
    for f in FILES:
        assert open(synthetic / ("auto." + f), "rb").read() == open(synthetic / ("a." + f), "rb").read(), f
    # ... and checked as a run of its own: the earlier lines, the four files, the model under the estimate
    with_and_without(synthetic, ["-e", "auto"], est_cov=n)
