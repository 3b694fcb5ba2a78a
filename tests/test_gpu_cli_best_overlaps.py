"""GPU: `raft --overlap-ends H [--ends-min-ratio F] --best-overlaps` -- PREFIX.best_overlaps.tsv and the option's stdout line against
the numpy restatement of tests/test_gpu_best_overlaps.py over ``hostio.load_paf(strand=True)``, with the reads that overlap_ends finds
contained left out; the reference's four files, overlap_ends.tsv and the rest of stdout byte for byte those of a run without the
flag; beside --min-identity / --min-overlap everything equal to a run on the text filtered in Python; beside -e auto, --read-stats,
two contexts and two ranks.  The set is the 300-read set of tests/test_gpu_cli_overlap_ends.py, built by that module's fixture."""
import os
import re

import pytest
from test_gpu_best_overlaps import want_best
from test_gpu_cli_overlap_ends import CMD, FILES, FILTER_LINE, dataset, files_of, run, strip_timing  # noqa: F401 (dataset: the fixture)
from test_gpu_cli_overlap_ends import LINE as ENDS_LINE
from test_gpu_overlap_ends import want_all

from raft_amd import hostio

pytestmark = pytest.mark.gpu
LINE = "INFO, best_overlaps(), "
NEW = ("overlap_ends.tsv", "best_overlaps.tsv")


def expected(d, paf, names, rl, H, F, masked=True):
    """-> the bytes of PREFIX.best_overlaps.tsv, the stdout line and the summary, from the restatements over the tokenised file"""
    reads = hostio.Reads(str(d / "reads.fa"))
    cols, sym = hostio.load_paf(str(d / paf), reads, with_flag=True, strand=True)
    reads.close()
    status = want_all(rl, cols[:6], cols[6], H, F, bool(sym))[2]
    skip = (status == 1).astype("uint8") if masked else None
    partner, span, flags, s = want_best(rl, cols[:6], cols[6], H, F, bool(sym), skip)
    lines = []
    for r, name in enumerate(names):
        f = [name, str(int(rl[r]))]
        for e in range(2):
            p, bits = int(partner[r, e]), int(flags[r]) >> (2 * e)
            f += ["*", "*", "0", "0"] if p < 0 else [names[p], "-" if bits & 1 else "+", str(int(span[r, e])), "1" if bits & 2 else "0"]
        lines.append("\t".join(f + ["1" if flags[r] & 16 else "0"]) + "\n")
    line = (f"{LINE}records = {s['n_records']}, candidates = {s['candidates']}, left out = {s['left_out']}, ends with a best overlap = {s['ends_best']}, "
            f"mutual = {s['ends_mutual']}, reads with both ends mutual = {s['reads_both_mutual']}, reads without a best overlap = {s['reads_no_best']}, "
            f"reads left out = {s['reads_skipped']} of {len(names)}")
    return "".join(lines).encode(), line, s, (partner, span)


def split_out(out, want_line):
    """The option's line is the last one, behind overlap_ends'; -> stdout without it and without the timing lines."""
    lines = out.split("\n")
    assert lines[-1] == "" and lines[-2] == want_line and lines[-3].startswith(ENDS_LINE) and sum(l.startswith(LINE) for l in lines) == 1, (lines[-4:], want_line)
    return strip_timing("\n".join(lines[:-2] + [""]))


def test_the_set_says_something(dataset):
    d, names, rl = dataset
    _, _, s, (partner, span) = expected(d, "overlaps.paf", names, rl, 1000, 800)
    assert 1 <= s["reads_skipped"] <= 299 and s["ends_best"] > 0 and s["ends_mutual"] > 0, s
    # (as worked out on the CPU beforehand)
    assert (s["n_records"], s["reads_skipped"], s["ends_best"], s["ends_mutual"], s["reads_both_mutual"]) == (25236, 279, 38, 28, 8), s
    _, _, _, (plain_partner, plain_span) = expected(d, "overlaps.paf", names, rl, 1000, 800, masked=False)
    assert int(((plain_partner != partner) | (plain_span != span)).sum()) == 565          # what the mask changes


@pytest.mark.parametrize("H,F,args", [(1000, 800, ["--overlap-ends", "1000"]), (0, 500, ["--overlap-ends", "0", "--ends-min-ratio", "500"]),
                                      (200, 1000, ["--best-overlaps", "--ends-min-ratio", "1000", "--overlap-ends", "200"])], ids=["H1000", "H0_F500", "H200_F1000"])
def test_the_file_and_the_line_equal_the_restatement(dataset, H, F, args):
    d, names, rl = dataset
    tag = f"bh{H}f{F}"
    without = [a for a in args if a != "--best-overlaps"]
    rc, plain = run(d, ["-e", "20"] + without + ["-o", "b" + tag, "reads.fa", "overlaps.paf"])
    assert rc == 0 and LINE not in plain and ENDS_LINE in plain, plain
    rc, out = run(d, ["-e", "20"] + (args if args != without else args + ["--best-overlaps"]) + ["-o", "a" + tag, "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    want_file, want_line, _, _ = expected(d, "overlaps.paf", names, rl, H, F)
    assert split_out(out, want_line) == strip_timing(plain)
    assert files_of(d, "b" + tag) == sorted(FILES + NEW[:1]) and files_of(d, "a" + tag) == sorted(FILES + NEW)
    for f in files_of(d, "b" + tag):
        assert open(d / f"a{tag}.{f}", "rb").read() == open(d / f"b{tag}.{f}", "rb").read(), f
    assert open(d / f"a{tag}.best_overlaps.tsv", "rb").read() == want_file


def test_beside_the_filter_everything_equals_a_run_on_the_filtered_text(dataset):
    d, names, rl = dataset
    opts = ["--overlap-ends", "1000", "--best-overlaps"]
    rc, want = run(d, ["-e", "20"] + opts + ["-o", "bwf", "reads.fa", "kept.paf"])
    assert rc == 0, want
    rc, got = run(d, ["-e", "20", "--min-identity", "99", "--min-overlap", "500"] + opts + ["-o", "bgf", "reads.fa", "overlaps.paf"])
    assert rc == 0, got
    lines = got.split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith(FILTER_LINE)]
    assert len(at) == 1 and lines[at[0] - 1].startswith(CMD)
    want_file, want_line, s, _ = expected(d, "kept.paf", names, rl, 1000, 800)
    assert f", kept = {s['n_records']}," in lines[at[0]] and s["ends_best"] > 0
    assert strip_timing("\n".join(lines[:at[0]] + lines[at[0] + 1:])) == strip_timing(want) and lines[-2] == want_line
    assert files_of(d, "bgf") == files_of(d, "bwf") == sorted(FILES + NEW)
    for f in files_of(d, "bwf"):
        assert open(d / f"bgf.{f}", "rb").read() == open(d / f"bwf.{f}", "rb").read(), f
    assert open(d / "bgf.best_overlaps.tsv", "rb").read() == want_file


@pytest.mark.parametrize("extra,env,est", [(["--read-stats"], {}, "20"), ([], {}, "auto"), ([], {"RAFT_DEVICES": "0,0"}, "20"), ([], {"RAFT_RANKS": "2"}, "20")],
                         ids=["read_stats", "auto", "two_contexts", "two_ranks"])
def test_beside_the_other_options(dataset, extra, env, est):
    d, names, rl = dataset
    tag = "b" + re.sub(r"\W", "", "_".join(extra + list(env) + [est]))
    rc, plain = run(d, ["-e", est] + extra + ["--overlap-ends", "1000", "-o", "p" + tag, "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, plain
    rc, out = run(d, ["-e", est] + extra + ["--overlap-ends", "1000", "--best-overlaps", "-o", "e" + tag, "reads.fa", "overlaps.paf"], **env)
    assert rc == 0, out
    want_file, want_line, _, _ = expected(d, "overlaps.paf", names, rl, 1000, 800)
    assert split_out(out, want_line) == strip_timing(plain)
    assert files_of(d, "e" + tag) == sorted(files_of(d, "p" + tag) + ["best_overlaps.tsv"])
    for f in files_of(d, "p" + tag):
        assert open(d / f"e{tag}.{f}", "rb").read() == open(d / f"p{tag}.{f}", "rb").read(), f
    assert open(d / f"e{tag}.best_overlaps.tsv", "rb").read() == want_file


@pytest.mark.parametrize("bad", [["--best-overlaps"], ["--best-overlaps", "--ends-min-ratio", "800"], ["--overlap-ends", "1000", "--best-overlaps=1"],
                                 ["--best-overlaps=1"]], ids=lambda b: " ".join(b))
def test_the_flag_alone_or_with_a_value_is_the_usage_error(tmp_path, bad):
    rc, out = run(tmp_path, ["-e", "3"] + bad + ["reads.fa", "overlaps.paf"])
    assert rc == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>\n" in out, out
    assert os.listdir(tmp_path) == []
