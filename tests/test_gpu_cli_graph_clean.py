"""GPU: `raft --overlap-ends H --string-graph --graph-clean [--clean-min-ratio W] [--clean-tip-reads T] [--clean-rounds R]` --
PREFIX.clean.tsv, PREFIX.clean.string_graph.gfa and .tsv, PREFIX.clean.unitigs.tsv and .layout.tsv and the option's two stdout lines
against the Python writers over the plain-Python rule of tests/cln_testlib.py over the edge list of tests/sg_testlib.py's oracle, and
the walk of tests/unitig_testlib.py over the cleaned table; without the flag every file and all of stdout those of the same command;
beside every other option the two lines are the last.  On the 300-read, 30-fold set of tests/test_gpu_cli_lift.py.  Every run goes
under a time limit of its own, and nothing more is started after one that aborted, faulted or ran into it."""
import numpy as np
import pytest
from cln_testlib import clean
from test_gpu_cli_all_options import ROWS
from test_gpu_cli_lift import dataset  # noqa: F401  (the fixture)
from test_gpu_cli_overlap_ends import FILES, files_of, strip_timing
from test_gpu_cli_string_graph import ENDS, EST, run
from test_gpu_cli_string_graph import OURS as GRAPH_FILES
from test_gpu_cli_string_graph import expected as graph_expected
from test_graph_clean_writer import clean_text
from test_string_graph_writer import gfa_text, tsv_text
from unitig_testlib import files_of as unitig_files
from unitig_testlib import stdout_line, walk

pytestmark = pytest.mark.gpu
LINE, UNITIGS_LINE = "INFO, graph_clean(), ", "INFO, graph_clean_unitigs(), "
OURS = ("clean.tsv", "clean.string_graph.gfa", "clean.string_graph.tsv", "clean.unitigs.tsv", "clean.unitigs.layout.tsv")
GRAPH = ["--overlap-ends", "100", "--string-graph"]


def expected(d, names, rl, W=500, T=4, R=3):
    """-> the bytes of the five files by name, the two stdout lines and the oracle's result"""
    g = graph_expected(d, "reads.fa", "overlaps.paf")[3]
    skip = (np.asarray(g["flags"]) & 16 != 0).astype(np.uint8)             # (string_graph's flagged reads: the contained ones)
    c = clean(rl, g["edge_u"], g["edge_w"], g["edge_span"], skip=skip, W=W, T=T, R=R)
    assert c["error_index"] == -1
    live = c["edge_state"] == 0
    graph = dict(arcs=c["arcs"], kept=c["kept"], flags=c["flags"], edge_u=g["edge_u"][live], edge_w=g["edge_w"][live], edge_span=g["edge_span"][live])
    w = walk(rl, c["partner"], c["span"], c["flags"])
    table, layout = unitig_files(w, names, rl)
    lengths = np.asarray(rl).tolist()
    files = {"clean.tsv": clean_text(names, lengths, c), "clean.string_graph.gfa": gfa_text(names, lengths, graph),
             "clean.string_graph.tsv": tsv_text(names, lengths, graph), "clean.unitigs.tsv": table, "clean.unitigs.layout.tsv": layout}
    s = c["summary"]
    line = (f"{LINE}min_ratio = {W} per mille, tip_reads = {T}, rounds = {s['rounds_run']} of {R}, converged = {s['converged']}, edges = {s['edges']}, "
            f"weak edges = {s['weak_edges']}, tips = {s['tips']}, tip reads = {s['tip_reads']}, tip bases = {s['tip_bases']}, tip edges = {s['tip_edges']}, "
            f"kept edges = {s['kept_edges']}, ends that branch = {s['ends_kept_more']}, dead ends = {s['ends_dead']}, "
            f"short isolated chains = {s['isolated_short']}")
    return {k: v.encode() for k, v in files.items()}, line, UNITIGS_LINE + stdout_line(w)[len("INFO, unitigs(), "):], c


def check_run(d, prefix, out, want):
    files, line, unitigs_line, _ = want
    lines = out.split("\n")
    assert lines[-1] == "" and lines[-3] == line and lines[-2] == unitigs_line, (lines[-4:], line, unitigs_line)
    assert sum(l.startswith(LINE) for l in lines) == 1 and sum(l.startswith(UNITIGS_LINE) for l in lines) == 1
    for f, text in files.items():
        assert open(d / f"{prefix}.{f}", "rb").read() == text, f


def test_the_files_and_the_lines_equal_the_oracle(dataset):  # noqa: F811
    d, names, rl = dataset
    _, out = run(d, ["-e", EST] + GRAPH + ["--graph-clean", "-o", "ca", "reads.fa", "overlaps.paf"])
    want = expected(d, names, rl)
    check_run(d, "ca", out, want)
    assert files_of(d, "ca") == sorted(FILES + ENDS + GRAPH_FILES + OURS)
    # without the flag: every file and all of stdout, byte for byte
    _, plain = run(d, ["-e", EST] + GRAPH + ["-o", "cb", "reads.fa", "overlaps.paf"])
    assert LINE not in plain and strip_timing("\n".join(out.split("\n")[:-3] + [""])) == strip_timing(plain)
    assert files_of(d, "cb") == sorted(FILES + ENDS + GRAPH_FILES)
    for f in FILES + ENDS + GRAPH_FILES:
        assert open(d / f"ca.{f}", "rb").read() == open(d / f"cb.{f}", "rb").read(), f


@pytest.mark.parametrize("W, T, R", [(1000, 2, 1), (0, 0, 64), (900, 2147483647, 2)])
def test_the_parameters(dataset, W, T, R):  # noqa: F811
    d, names, rl = dataset
    prefix = f"cp{W}_{R}"
    _, out = run(d, ["-e", EST] + GRAPH + ["--graph-clean", "--clean-min-ratio", str(W), "--clean-tip-reads", str(T), "--clean-rounds", str(R), "-o", prefix,
                     "reads.fa", "overlaps.paf"])
    want = expected(d, names, rl, W, T, R)
    check_run(d, prefix, out, want)
    s = want[3]["summary"]
    if W == 0:                                                             # (nothing is cut and nothing is a candidate: the graph of --string-graph)
        assert (s["weak_edges"], s["tips"], s["rounds_run"], s["converged"], s["kept_edges"]) == (0, 0, 1, 1, s["edges"])
        assert want[0]["clean.string_graph.gfa"] == graph_expected(d, "reads.fa", "overlaps.paf")[0]
    else:
        assert s["weak_edges"] >= 1 and s["kept_edges"] >= 1, s


def test_beside_every_other_option_the_two_lines_are_the_last(dataset):  # noqa: F811
    d, names, rl = dataset
    every = [a for _, args, _ in ROWS for a in args] + ["--components", "--string-graph", "--containment"]
    _, out = run(d, ["-e", EST] + every + ["--graph-clean", "-o", "c_all", "reads.fa", "overlaps.paf"])
    check_run(d, "c_all", out, expected(d, names, rl))
    _, without = run(d, ["-e", EST] + every + ["-o", "c_none", "reads.fa", "overlaps.paf"])
    assert strip_timing("\n".join(out.split("\n")[:-3] + [""])) == strip_timing(without)
    assert sorted(set(files_of(d, "c_all")) - set(files_of(d, "c_none"))) == sorted(OURS)
    for f in files_of(d, "c_none"):
        assert open(d / f"c_all.{f}", "rb").read() == open(d / f"c_none.{f}", "rb").read(), f
