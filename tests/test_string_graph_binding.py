"""CPU: the functions of include/raft_hip_sg.h and include/raft_host_sg.h are declared by their bindings (``SG_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; the summary is seventeen int64; exports_sg.map
names the three entry points and nothing of the other tables, and libraft_hip_sg.so exports exactly them.  The table of the nine side
libraries is what it was and this library is a row of the one beside it; the two Makefile lines.  What ``Engine.string_graph`` hands to
the library, against the recording stand-in of tests/test_binding_calls.py."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from raft_testlib import ROOT
from test_binding_calls import CTX, SIDE_TAGS, Lib, T, make_engine, side_library
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_sg.h", "raft_hip_", engine), ("raft_host_sg.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_sg_abi", "raft_hip_string_graph_device", "raft_hip_string_graph_host"]
HOST_FUNCTIONS = ["raft_host_write_string_graph"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI", "FLT_ABI", "END_ABI", "BEST_ABI", "UTG_ABI", "LIFT_ABI", "CC_ABI")
SUMMARY = ["records", "dovetail_views", "views_left_out", "arcs", "duplicate_arcs", "unpaired_arcs", "reducible_arcs", "edges", "removed_edges",
           "kept_edges", "ends_with_arc", "ends_kept_one", "ends_kept_more", "ends_mutual", "ends_dead", "reads_flagged", "longest_row"]
PER_READ = ["arcs", "kept", "partner", "span", "flags"]
EDGES = ["edge_u", "edge_w", "edge_span", "edge_ext", "edge_back", "edge_flags"]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_sg", "raft_host_sg"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.SG_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.SG_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_three_entry_points_the_summary_and_the_flags():
    assert sorted(header_functions("raft_hip_sg.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.SG_ABI)
    assert sorted(header_functions("raft_host_sg.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.SG_ABI)
    raw = open(os.path.join(ROOT, "include", "raft_hip_sg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef struct raft_hip_sg_summary \{(.*?)\}", text, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
    assert fields == [n for n, _ in engine._SgSummary._fields_] == SUMMARY
    assert all(t is C.c_int64 for _, t in engine._SgSummary._fields_) and C.sizeof(engine._SgSummary) == 8 * 17
    # the two forms take the same parameters: the context, the nine of the columns, strand, skip, H, F, symmetric, fuzz, emit_removed,
    # out_cap, eleven outputs, n_out, the summary, error_index, the seconds, the launches
    dev, host = (header_functions("raft_hip_sg.h", "raft_hip_")[n] for n in ENTRY_POINTS[1:])
    assert dev == host and len(dev[1]) == 34
    # ... those of raft_hip_best_overlaps_* up to symmetric; then fuzz, emit_removed and the capacity
    best = header_functions("raft_hip_best.h", "raft_hip_")["raft_hip_best_overlaps_device"][1]
    assert dev[1][:15] == best[:15] and dev[1][15:18] == ["int32", "int32", "int64"]
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define RAFT_HIP_SG_EDGE_([A-Z_]+)\s+(\d+)\b", text, flags=re.M)}
    assert flags == {"RED_U": engine.SG_EDGE_RED_U, "RED_W": engine.SG_EDGE_RED_W, "UNPAIRED": engine.SG_EDGE_UNPAIRED} and sorted(flags.values()) == [1, 2, 4]
    assert list(engine.SG_EDGE_COLUMNS) == EDGES


def test_the_nine_stay_and_the_library_is_a_row_beside_them():
    assert list(engine._SIDE) == SIDE_TAGS and len(engine._SIDE) == 9
    assert engine._SIDE_LATER["sg"] == ("libraft_hip_sg.so", engine.SG_ABI, "raft_hip_sg_abi")
    assert list(engine._SIDE_LATER) == ["cc", "sg"] and not (set(engine._SIDE) & set(engine._SIDE_LATER))
    rows = list(engine._SIDE.values()) + list(engine._SIDE_LATER.values())
    assert all(len(row) == 3 for row in rows) and len({row[0] for row in rows}) == len(rows) == len({row[2] for row in rows})
    for tag, (file, abi, abi_fn) in engine._SIDE_LATER.items():
        assert file == f"libraft_hip_{tag}.so" and abi_fn == f"raft_hip_{tag}_abi" and abi_fn in abi
    makefile = open(os.path.join(ROOT, "raft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SIDE \+= sg=string_graph_lib$", makefile, flags=re.M)
    assert makefile.index("\nSIDE += cc=components_lib") < makefile.index("\nSIDE += sg=string_graph_lib") < makefile.index("\nSIDE_TAGS =")
    host = open(os.path.join(ROOT, "raft_amd", "host", "Makefile")).read()
    side = re.search(r"^SIDE = (.*)$", host, flags=re.M).group(1).split()
    assert side[:2] == ["cc", "lift"] and "sg" in side and len(side) == len(set(side)) == 11 and "$(SIDE:%=-lraft_hip_%)" in host
    assert all(os.path.exists(os.path.join(ROOT, "include", h)) for h in ("raft_host_sg.h", "raft_hip_sg.h"))
    assert all(os.path.exists(os.path.join(ROOT, "raft_amd", "csrc", f)) for f in ("string_graph.hpp", "string_graph_rule.hpp", "string_graph_lib.hip", "exports_sg.map"))
    # its buffers are one more entry in the list of a context's resources
    ctx = open(os.path.join(ROOT, "raft_amd", "csrc", "engine_ctx.hpp")).read()
    assert re.search(r"^\s*DevBufSet<kSgBufs> sg\{bufs\};", ctx, flags=re.M)


def test_load_side_library_finds_it(monkeypatch):
    opened = []

    class Opened:
        def __init__(self, path):
            opened.append(os.path.basename(path))

        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return lambda *a: 11
    monkeypatch.setattr(engine, "_side_libs", {})
    monkeypatch.setattr(engine, "load_library", lambda: Opened("libraft_hip.so"))
    monkeypatch.setattr(engine.C, "CDLL", Opened)
    monkeypatch.setattr(engine.os.path, "exists", lambda p: True)
    lib = engine.load_side_library("sg")
    assert engine.load_side_library("sg") is lib and [o for o in opened if o != "libraft_hip.so"] == ["libraft_hip_sg.so"]


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("string_graph" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and not any("string_graph" in n for n in hostio.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())


def _exported(file):
    path = os.path.join(os.path.dirname(engine._LIB_PATH), file)
    assert os.path.exists(path)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_sg.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    if shutil.which("nm") is not None:
        assert _exported("libraft_hip_sg.so") == ENTRY_POINTS
        assert _exported("libraft_hip_cc.so") == ["raft_hip_cc_abi", "raft_hip_components_device", "raft_hip_components_host"]


# ---- what Engine.string_graph hands over: three reads, four records
RL = np.array([100, 250, 49], np.int32)
QID, QS, QE = np.array([0, 1, 1, 2], np.int32), np.array([0, 10, 20, 0], np.int32), np.array([90, 200, 240, 49], np.int32)
TID, TS, TE = np.array([1, 0, 2, 1], np.int32), np.array([5, 0, 1, 2], np.int32), np.array([95, 99, 40, 50], np.int32)
STRAND, SKIP = np.array([0, 1, 0, 1], np.uint8), np.array([0, 0, 1], np.uint8)
HOST = dict(rl=RL, qid=QID, qs=QS, qe=QE, tid=TID, ts=TS, te=TE, strand=STRAND, skip=SKIP)
D = {k: T(0x10000 * (i + 1), 3 if k == "rl" else 4) for i, k in enumerate(("rl", "qid", "qs", "qe", "tid", "ts", "te"))}
D["strand"], D["skip"] = T(0x80000, 4, torch.uint8), T(0x90000, 3, torch.uint8)
NAMES = {**{a.ctypes.data: k for k, a in HOST.items()}, **{t.ptr: "d_" + k for k, t in D.items()}}
COLS = ("rl", "qid", "qs", "qe", "tid", "ts", "te", "strand")


def call(monkeypatch, *args, **kw):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("sg", side))
    res = eng.string_graph(*args, **kw)
    assert len(side.calls) == 1 and eng._lib.lib_calls() == []          # (the stand-in's n_out is 0: the size query is all there is)
    return eng, side.calls[0], res


def check_outputs(res, args, n_reads=3):
    """The five per-read arrays the library writes are the ones the result holds; the size query hands over no edge array"""
    for key, address in zip(PER_READ, args[18:23]):
        assert res[key].dtype == (np.uint8 if key == "flags" else np.int32) and res[key].shape == ((n_reads,) if key == "flags" else (n_reads, 2)), key
        assert address != 0 and (res[key].size == 0 or res[key].ctypes.data == address), key
    assert args[23:29] == [0] * 6 and all(res[k].shape == (0,) for k in EDGES) and res["edge_flags"].dtype == np.uint8 and res["edge_u"].dtype == np.int32
    assert args[29] == ("i64", 0) and args[30] == ("_SgSummary", dict.fromkeys(SUMMARY, 0))
    assert args[31] == ("i64", -1) and args[32] == ("f64", 0.0) and args[33] == ("i64", 0)
    assert sorted(res) == sorted(PER_READ + EDGES + ["n_out", "summary", "kernel_seconds", "launches"])
    assert res["summary"] == dict.fromkeys(SUMMARY, 0) and res["kernel_seconds"] == 0.0 and res["launches"] == 0 and res["n_out"] == 0


def test_the_host_form_and_the_defaults(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *[HOST[k] for k in COLS])
    assert name == "raft_hip_string_graph_host" and len(args) == 34
    assert args[:12] == ["ctx", 3, "rl", 4, "qid", "qs", "qe", "tid", "ts", "te", "strand", 0]
    assert args[12:18] == [1000, 800, 0, 1000, 0, 0]
    check_outputs(res, args)
    assert eng._lib.calls == []                                       # (no torch stream for host arrays)


def test_the_device_form_and_the_parameters(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *[D[k] for k in COLS], max_overhang=7, min_ratio_permille=900, fuzz=12, symmetric=True, skip=D["skip"],
                                  emit_removed=True)
    assert name == "raft_hip_string_graph_device" and len(args) == 34
    assert args[:12] == ["ctx", 3, "d_rl", 4, "d_qid", "d_qs", "d_qe", "d_tid", "d_ts", "d_te", "d_strand", "d_skip"]
    assert args[12:18] == [7, 900, 1, 12, 1, 0]
    check_outputs(res, args)
    assert eng._lib.calls == [("use_torch_stream", [])]
    assert eng.last_string_graph_launches == 0 and eng.last_string_graph_seconds == 0.0
    _, (_, args), _ = call(monkeypatch, *[HOST[k] for k in COLS], skip=SKIP, fuzz=0)
    assert args[11] == "skip" and args[15] == 0
    with pytest.raises(TypeError):                                    # keyword-only behind strand
        make_engine(NAMES).string_graph(*[HOST[k] for k in COLS], 5)


def test_the_edge_list_is_sized_by_asking_twice(monkeypatch):
    eng = make_engine(NAMES)

    class Five(Lib):
        def __getattr__(self, name):
            fn = super().__getattr__(name)

            def wrapped(*args):
                rc = fn(*args)
                args[29]._obj.value = 5
                return rc
            return wrapped
    side = Five(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("sg", side))
    res = eng.string_graph(*[HOST[k] for k in COLS])
    assert len(side.calls) == 2 and res["n_out"] == 5 and all(res[k].shape == (5,) for k in EDGES)
    (_, first), (_, second) = side.calls
    assert first[17] == 0 and first[23:29] == [0] * 6 and second[17] == 5
    assert second[23:29] == [res[k].ctypes.data for k in EDGES] and second[18:23] == first[18:23] and second[:17] == first[:17]


def test_no_reads_and_no_records(monkeypatch):
    empty, none = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    _, (name, args), res = call(monkeypatch, empty, *[empty] * 6, none)
    assert name == "raft_hip_string_graph_host" and args[:12] == ["ctx", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert all(res[k].size == 0 for k in PER_READ + EDGES)


def test_what_is_refused_before_any_call(monkeypatch):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("sg", side))
    host = [HOST[k] for k in COLS]
    with pytest.raises(ValueError, match="string_graph needs read_len, the six columns and strand"):
        eng.string_graph(*host[:7], None)
    with pytest.raises(ValueError, match="string_graph needs"):
        eng.string_graph(*host[:5], None, *host[6:])
    with pytest.raises(ValueError, match="differ in length"):
        eng.string_graph(*host[:7], STRAND[:3])
    with pytest.raises(ValueError, match="skip is one byte per read"):
        eng.string_graph(*host, skip=SKIP[:2])
    dev = [D[k] for k in COLS]
    with pytest.raises(TypeError, match="strand as a contiguous uint8"):
        eng.string_graph(*dev[:7], T(0x80000, 4, torch.int32))
    with pytest.raises(TypeError, match="contiguous int32 CUDA"):
        eng.string_graph(*dev[:6], T(0x70000, 4, torch.int64), dev[7])
    assert side.calls == [] and eng._lib.lib_calls() == []
    assert eng._ctx.value == CTX
