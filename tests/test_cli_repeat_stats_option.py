"""CPU: `raft --repeat-stats` takes no argument: `--repeat-stats=3` is rejected the way any bad option is -- the usage text on stdout,
exit code 1, before any device is asked for --, and the plain option passes the parser: the run gets as far as the device (where there
is none, the engine's device error is its last line; where there is one, the job runs and the option's line is the last)."""
import os
import re
import subprocess

from raft_testlib import ROOT
from test_cli_early_exits import PAF, READS, USAGE

RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")
LINE = re.compile(r"INFO, repeat_stats\(\), repeats = (\d+), interior = (\d+), spanned = (\d+), interior spanned = (\d+), untouched = (\d+), "
                  r"sides inside a repeat = (\d+)$")


def run(tmp_path, *options):
    (tmp_path / "a.fa").write_text(READS)
    (tmp_path / "b.paf").write_text(PAF)
    return subprocess.run([RAFT, "-e", "30", *options, "a.fa", "b.paf"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_an_argument_prints_the_usage(tmp_path):
    r = run(tmp_path, "--repeat-stats=3")
    assert r.returncode == 1, r.stdout.decode() + r.stderr.decode()
    assert r.stdout.decode() == USAGE
    assert sorted(os.listdir(tmp_path)) == ["a.fa", "b.paf"]          # (not even the output FASTA is created)


def test_the_plain_option_reaches_the_device(tmp_path):
    for options in (("--repeat-stats",), ("--fragment-overlaps", "--repeat-stats"), ("--repeat-stats", "--fragment-overlaps")):
        r = run(tmp_path, *options)
        out = r.stdout.decode()
        assert "Usage:" not in out and out.startswith("INFO, printParams(), reso = 50\n")
        lines = out.split("\n")
        if r.returncode == 0:
            m = LINE.match(lines[-2])
            assert m and os.path.exists(tmp_path / "raft.long_repeats.stats.tsv"), lines[-2]
            runs, interior, spanned, both, untouched, _ = (int(x) for x in m.groups())
            assert both <= min(interior, spanned) <= runs and untouched <= runs
            assert len(options) == 1 or lines[-3].startswith("INFO, fragment_overlaps(), fragments = ")       # behind that line, whatever the order
        else:
            assert r.returncode == 1 and lines[-2].startswith("ERROR, raft_hip_create(), device 0: "), out
            assert not os.path.exists(tmp_path / "raft.long_repeats.stats.tsv")


def test_the_line_is_the_plan_header_s(tmp_path):
    """The words of the stdout line are repeat_stats_line's, in cli_plan.hpp beside fragment_overlaps_line."""
    text = open(os.path.join(ROOT, "raft_amd", "host", "cli_plan.hpp")).read()
    assert text.index("inline std::string fragment_overlaps_line(") < text.index("inline std::string repeat_stats_line(")
    for words in ("INFO, repeat_stats(), repeats = ", ", interior = ", ", spanned = ", ", interior spanned = ", ", untouched = ", ", sides inside a repeat = "):
        assert f'"{words}"' in text, words
