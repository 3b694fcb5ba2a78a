"""GPU: every optional output of `raft` at once equals each of them alone.  On the 300-read, 30-fold set of tests/test_gpu_cli_lift.py,
`raft -e 30` with every option on is compared with one run per option (that option and what it needs: --best-overlaps with
--overlap-ends, --unitigs with both): every file of the combined run is byte for byte the same-named file of the single run, the
option's stdout line is the same line, and the combined run's lines stand behind the `CMD:` line in the one order the command line
keeps for running, writing and reporting.  Four conditions, combined against single under the same one: plain; beside the filter;
RAFT_CLI_PREPARE=1, where the window records are written over the query column that three of the options read after the job; two
contexts.  Every run goes under a time limit of its own, and nothing more is started after one that aborted, faulted or ran into it."""
import os
import subprocess

import pytest
from test_gpu_cli_lift import dataset  # noqa: F401  (the fixture)
from test_gpu_cli_overlap_ends import CMD, FILES, RAFT, files_of

pytestmark = pytest.mark.gpu
EST = "30"
# the options in the order of the command line's table (raft_main.cpp kExtras; the filter's row comes first, with the condition):
# name of the stdout line, arguments, files
ROWS = (("read_stats", ["--read-stats"], ("read_stats.tsv",)),
        ("low_coverage", ["--low-cov", "2"], ("low_coverage.bed",)),
        ("repeat_overlaps", ["--repeat-overlaps", "500"], ("repeat_overlaps.tsv", "repeat_overlaps.records.tsv")),
        ("fragment_overlaps", ["--fragment-overlaps"], ("fragments.tsv",)),
        ("repeat_stats", ["--repeat-stats"], ("long_repeats.stats.tsv",)),
        ("overlap_ends", ["--overlap-ends", "100"], ("overlap_ends.tsv",)),
        ("best_overlaps", ["--best-overlaps"], ("best_overlaps.tsv",)),
        ("unitigs", ["--unitigs"], ("unitigs.tsv", "unitigs.layout.tsv")),
        ("fragment_paf", ["--fragment-paf"], ("fragments.paf",)))
NEEDS = {"best_overlaps": ("overlap_ends",), "unitigs": ("overlap_ends", "best_overlaps")}
CONDITIONS = {"plain": ([], {}), "filter": (["--min-identity", "99", "--min-overlap", "500"], {}), "cli_prepare": ([], {"RAFT_CLI_PREPARE": "1"}),
              "two_contexts": ([], {"RAFT_DEVICES": "0,0"})}
FATAL = (134, 139, 124, 137)          # abort, segmentation fault, the time limit (and its kill)
stopped = []                          # the run after which nothing more is started


def run(d, args, env):
    if stopped:
        pytest.fail(f"not started: an earlier run ended with {stopped[0]}")
    r = subprocess.run(["timeout", "-k", "10", "60", RAFT] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, RAFT_TIMING="1", **env))
    if r.returncode in FATAL:
        stopped.append(f"exit code {r.returncode}: raft {' '.join(args)} under {env}")
        pytest.fail(stopped[0] + "\n" + r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:])
    assert r.returncode == 0, (args, env, r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    return r.stdout.decode().split("\n"), r.stderr.decode()


def option_lines(lines):
    """The lines behind the `CMD:` line, which is followed by nothing but the options' lines: -> [(name, line)]"""
    at = [i for i, l in enumerate(lines) if l.startswith(CMD)]
    assert len(at) == 1 and lines[-1] == "", lines[-12:]
    rest = lines[at[0] + 1:-1]
    assert all(l.startswith("INFO, ") and "(), " in l for l in rest), rest
    return [(l[len("INFO, "):l.index("(), ")], l) for l in rest]


@pytest.mark.parametrize("condition", list(CONDITIONS))
def test_all_at_once_equals_one_at_a_time(dataset, condition):  # noqa: F811
    d = dataset[0]
    extra, env = CONDITIONS[condition]
    head = ["filter_overlaps"] if condition == "filter" else []
    every = [a for _, args, _ in ROWS for a in args]
    lines, err = run(d, ["-e", EST] + extra + every + ["-o", f"all_{condition}", "reads.fa", "overlaps.paf"], env)
    got = option_lines(lines)
    assert [n for n, _ in got] == head + [n for n, _, _ in ROWS], got                    # the table's order
    assert files_of(d, f"all_{condition}") == sorted(FILES + tuple(f for _, _, fs in ROWS for f in fs))
    if condition == "cli_prepare":
        assert " input windows " in err, err                                             # (the query column was written over)
    combined = dict(got)
    for name, args, files in ROWS:
        needed = [r for r in ROWS if r[0] in NEEDS.get(name, ())]
        prefix = f"{name}_{condition}"
        one, _ = run(d, ["-e", EST] + extra + [a for r in needed for a in r[1]] + args + ["-o", prefix, "reads.fa", "overlaps.paf"], env)
        single = option_lines(one)
        assert [n for n, _ in single] == head + [r[0] for r in needed] + [name], single
        for n, line in single:
            assert combined[n] == line, (condition, name, n)
        want_files = sorted(FILES + tuple(f for r in needed for f in r[2]) + files)
        assert files_of(d, prefix) == want_files, (condition, name)
        for f in want_files:
            assert open(d / f"{prefix}.{f}", "rb").read() == open(d / f"all_{condition}.{f}", "rb").read(), (condition, name, f)
