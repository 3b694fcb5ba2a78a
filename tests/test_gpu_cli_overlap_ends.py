"""GPU: `raft --overlap-ends H [--ends-min-ratio F]` -- PREFIX.overlap_ends.tsv and the option's stdout line against the numpy
restatement of tests/test_gpu_overlap_ends.py over ``hostio.load_paf(strand=True)``; the reference's four files and the rest of stdout
byte for byte those of a run without the option; beside --min-identity / --min-overlap everything equal to a run on the text filtered
in Python; beside -e auto, --read-stats, two contexts and two ranks.  The set: 300 synthetic reads, a symmetric PAF on both strands
(the strand chosen by pair of reads) in which every kind of a valid record between two reads occurs -- invalid coordinates end a job
before it writes anything, so they are the kernel test's business."""
import os
import re
import subprocess

import numpy as np
import pytest
from raft_testlib import ROOT, write_fasta
from test_gpu_cli_filter import keeps
from test_gpu_overlap_ends import KIND_NAMES, want_all

from raft_amd import hostio

pytestmark = pytest.mark.gpu
RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")
FILES = ("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed")
LINE = "INFO, overlap_ends(), "
FILTER_LINE = "INFO, filter_overlaps(), "
CMD = "INFO, main(), CMD:"
P, L = 990, 500


def run(cwd, args, **env):
    r = subprocess.run([RAFT] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, **env))
    return r.returncode, r.stdout.decode()


def strip_timing(out):
    return "\n".join(l for l in out.split("\n") if not l.startswith("INFO, main(), program completed after") and not l.startswith(CMD))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from raft_amd.synth import make_overlaps
    d = tmp_path_factory.mktemp("ends_cli")
    o = make_overlaps(300, coverage=30, seed=5)
    rl = o.read_len.numpy()
    qid, qs, qe, tid, ts, te = (c.numpy().astype(np.int64) for c in o.columns())
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(d / "reads.fa", names, rl)
    pair = (np.minimum(qid, tid) * 2 ** 20 + np.maximum(qid, tid)) * 7919 + 13          # (a record and its mirror agree)
    rev = (pair // 41) % 2
    block = np.maximum(qe - qs, te - ts) + 3
    matches = -(-block * (975 + pair % 26) // 1000)
    lines = ["\t".join([names[qid[i]], str(rl[qid[i]]), str(qs[i]), str(qe[i]), "+-"[rev[i]], names[tid[i]], str(rl[tid[i]]), str(ts[i]), str(te[i]),
                        str(matches[i]), str(block[i]), "60"]) for i in range(qid.size)]
    kept = [l for l in lines if keeps(l, P, L)]
    assert 0.2 * len(lines) < len(kept) < 0.9 * len(lines)
    (d / "overlaps.paf").write_text("".join(l + "\n" for l in lines))
    (d / "kept.paf").write_text("".join(l + "\n" for l in kept))
    return d, names, rl


def expected(d, paf, names, rl, H, F):
    """-> the bytes of PREFIX.overlap_ends.tsv and the stdout line, from the restatement over the tokenised file"""
    reads = hostio.Reads(str(d / "reads.fa"))
    cols, sym = hostio.load_paf(str(d / paf), reads, with_flag=True, strand=True)
    reads.close()
    kinds, counts, status, s = want_all(rl, cols[:6], cols[6], H, F, bool(sym))
    text = "".join("\t".join([names[r], str(int(rl[r]))] + [str(int(counts[k, r])) for k in range(5)] + [str(int(status[r]))]) + "\n" for r in range(len(names)))
    line = (f"{LINE}max_overhang = {H}, min_ratio = {F} per mille, records = {s['n_records']}, internal = {s['kind_internal']}, "
            f"query contained = {s['kind_query_contained']}, target contained = {s['kind_target_contained']}, dovetail = {s['kind_end3'] + s['kind_end5']}, "
            f"self = {s['kind_self']}, invalid = {s['kind_invalid']}, contained reads = {s['reads_contained']}, "
            f"dead ends = {s['reads_dead5'] + s['reads_dead3']}, isolated reads = {s['reads_isolated']} of {len(names)}")
    return text.encode(), line, s, cols[6]


def split_out(out, want_line):
    """The option's line is the last one; -> stdout without it and without the timing lines."""
    lines = out.split("\n")
    assert lines[-1] == "" and lines[-2] == want_line and sum(l.startswith(LINE) for l in lines) == 1, (lines[-4:], want_line)
    return strip_timing("\n".join(lines[:-2] + [""]))


def files_of(d, prefix):
    return sorted(f[len(prefix) + 1:] for f in os.listdir(d) if f.startswith(prefix + "."))


def test_the_set_holds_both_strands_and_every_kind(dataset):
    d, names, rl = dataset
    _, _, s, strand = expected(d, "overlaps.paf", names, rl, 1000, 800)
    assert all(s[k] > 0 for k in KIND_NAMES[1:6]) and 0 < int(strand.sum()) < strand.size, s
    assert s["reads_contained"] > 0 and s["reads_linked"] > 0


@pytest.mark.parametrize("H,F,args", [(1000, 800, ["--overlap-ends", "1000"]), (0, 500, ["--overlap-ends", "0", "--ends-min-ratio", "500"]),
                                      (200, 1000, ["--ends-min-ratio", "1000", "--overlap-ends", "0200"])], ids=["H1000", "H0_F500", "H200_F1000"])
def test_the_file_and_the_line_equal_the_restatement(dataset, H, F, args):
    d, names, rl = dataset
    tag = f"h{H}f{F}"
    rc, plain = run(d, ["-e", "20", "-o", "b" + tag, "reads.fa", "overlaps.paf"])
    assert rc == 0 and LINE not in plain, plain
    rc, out = run(d, ["-e", "20"] + args + ["-o", "a" + tag, "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    want_file, want_line, _, _ = expected(d, "overlaps.paf", names, rl, H, F)
    assert split_out(out, want_line) == strip_timing(plain)
    assert files_of(d, "b" + tag) == sorted(FILES) and files_of(d, "a" + tag) == sorted(FILES + ("overlap_ends.tsv",))
    for f in FILES:
        assert open(d / f"a{tag}.{f}", "rb").read() == open(d / f"b{tag}.{f}", "rb").read(), f
    assert open(d / f"a{tag}.overlap_ends.tsv", "rb").read() == want_file


def test_beside_the_filter_everything_equals_a_run_on_the_filtered_text(dataset):
    d, names, rl = dataset
    rc, want = run(d, ["-e", "20", "--overlap-ends", "1000", "-o", "wf", "reads.fa", "kept.paf"])
    assert rc == 0, want
    rc, got = run(d, ["-e", "20", "--min-identity", "99", "--min-overlap", "500", "--overlap-ends", "1000", "-o", "gf", "reads.fa", "overlaps.paf"])
    assert rc == 0, got
    lines = got.split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith(FILTER_LINE)]
    assert len(at) == 1 and lines[at[0] - 1].startswith(CMD)
    want_file, want_line, s, _ = expected(d, "kept.paf", names, rl, 1000, 800)
    assert f", kept = {s['n_records']}," in lines[at[0]]
    assert strip_timing("\n".join(lines[:at[0]] + lines[at[0] + 1:])) == strip_timing(want) and lines[-2] == want_line
    assert files_of(d, "gf") == files_of(d, "wf") == sorted(FILES + ("overlap_ends.tsv",))
    for f in files_of(d, "wf"):
        assert open(d / f"gf.{f}", "rb").read() == open(d / f"wf.{f}", "rb").read(), f
    assert open(d / "gf.overlap_ends.tsv", "rb").read() == want_file


@pytest.mark.parametrize("extra,env,est", [(["--read-stats"], {}, "20"), ([], {}, "auto"), ([], {"RAFT_DEVICES": "0,0"}, "20"), ([], {"RAFT_RANKS": "2"}, "20")],
                         ids=["read_stats", "auto", "two_contexts", "two_ranks"])
def test_beside_the_other_options(dataset, extra, env, est):
    d, names, rl = dataset
    tag = re.sub(r"\W", "", "_".join(extra + list(env) + [est]))
    rc, plain = run(d, ["-e", est] + extra + ["-o", "p" + tag, "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, plain
    rc, out = run(d, ["-e", est] + extra + ["--overlap-ends", "1000", "-o", "e" + tag, "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, out
    want_file, want_line, _, _ = expected(d, "overlaps.paf", names, rl, 1000, 800)
    assert split_out(out, want_line) == strip_timing(plain)
    assert files_of(d, "e" + tag) == sorted(files_of(d, "p" + tag) + ["overlap_ends.tsv"])
    for f in files_of(d, "p" + tag):
        assert open(d / f"e{tag}.{f}", "rb").read() == open(d / f"p{tag}.{f}", "rb").read(), f
    assert open(d / f"e{tag}.overlap_ends.tsv", "rb").read() == want_file


@pytest.mark.parametrize("bad", [["--ends-min-ratio", "800"], ["--ends-min-ratio", "0"], ["--overlap-ends", "1000", "--ends-min-ratio", "1001"],
                                 ["--overlap-ends", "-1"], ["--overlap-ends", "2147483648"], ["--overlap-ends", "1k"], ["--overlap-ends", ""],
                                 ["--overlap-ends", "1000", "--ends-min-ratio", "80.0"]], ids=lambda b: " ".join(b))
def test_a_bad_value_or_the_ratio_alone_is_the_usage_error(tmp_path, bad):
    rc, out = run(tmp_path, ["-e", "3"] + bad + ["reads.fa", "overlaps.paf"])
    assert rc == 1 and out.startswith("Usage: raft [options] <input-reads.fa> <in.paf>\n"), out
    assert os.listdir(tmp_path) == []
