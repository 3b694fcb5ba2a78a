"""CPU: the functions of include/raft_hip_cln.h and include/raft_host_cln.h are declared by their bindings (``CLN_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; the summary is the header's int64 fields;
exports_cln.map names the three entry points and nothing of the other tables, and libraft_hip_cln.so exports exactly them.  The
library is a row of the open table, which ``load_side_library`` looks through behind the closed ones.  What ``Engine.graph_clean``
hands to the library, against the recording stand-in of tests/test_binding_calls.py."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from cln_testlib import ARRAYS, SUMMARY
from raft_testlib import ROOT
from test_binding_calls import CTX, Lib, T, make_engine, side_library
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_cln.h", "raft_hip_", engine), ("raft_host_cln.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_cln_abi", "raft_hip_graph_clean_device", "raft_hip_graph_clean_host"]
HOST_FUNCTIONS = ["raft_host_write_graph_clean"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI", "FLT_ABI", "END_ABI", "BEST_ABI", "UTG_ABI", "LIFT_ABI", "CC_ABI", "SG_ABI", "CTN_ABI")


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_cln", "raft_host_cln"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.CLN_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.CLN_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_entry_points_the_summary_and_the_flags():
    assert sorted(header_functions("raft_hip_cln.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.CLN_ABI)
    assert sorted(header_functions("raft_host_cln.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.CLN_ABI)
    raw = open(os.path.join(ROOT, "include", "raft_hip_cln.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef struct raft_hip_cln_summary \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"\b([a-z0-9_]+)\s*[,;]", body) == [n for n, _ in engine._ClnSummary._fields_] == SUMMARY
    assert all(t is C.c_int64 for _, t in engine._ClnSummary._fields_) and C.sizeof(engine._ClnSummary) == 8 * len(SUMMARY)
    fns = header_functions("raft_hip_cln.h", "raft_hip_")
    dev, host = fns["raft_hip_graph_clean_device"], fns["raft_hip_graph_clean_host"]
    assert dev == host and len(dev[1]) == 25
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define RAFT_HIP_CLN_([A-Z_]+)\s+(\d+)\b", text, flags=re.M)}
    assert flags == {"WEAK_U": engine.CLN_WEAK_U, "WEAK_W": engine.CLN_WEAK_W, "TIP": engine.CLN_TIP, "READ_STAYS": engine.CLN_READ_STAYS,
                     "READ_TIP": engine.CLN_READ_TIP, "READ_FLAGGED": engine.CLN_READ_FLAGGED}
    rule = open(os.path.join(ROOT, "raft_amd", "csrc", "graph_clean_rule.hpp")).read()
    assert int(re.search(r"kClnMaxRounds = (\d+)", rule).group(1)) == engine.CLN_MAX_ROUNDS == 64
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())


def test_the_library_is_a_row_of_the_open_table():
    assert engine._SIDE_OPEN["cln"] == ("libraft_hip_cln.so", engine.CLN_ABI, "raft_hip_cln_abi")
    assert not any("cln" in table for table in engine._SIDE_TABLES) and engine._SIDE_OPEN not in engine._SIDE_TABLES
    closed = [row for table in engine._SIDE_TABLES for row in table.values()]
    for tag, (file, abi, abi_fn) in engine._SIDE_OPEN.items():
        assert file == f"libraft_hip_{tag}.so" and abi_fn == f"raft_hip_{tag}_abi" and abi_fn in abi
        assert file not in [row[0] for row in closed] and abi_fn not in [row[2] for row in closed]
    makefile = open(os.path.join(ROOT, "raft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SIDE \+= cln=graph_clean_lib$", makefile, flags=re.M)
    assert makefile.index("\nSIDE += ctn=containment_lib") < makefile.index("\nSIDE += cln=graph_clean_lib") < makefile.index("\nSIDE_TAGS =")
    host = open(os.path.join(ROOT, "raft_amd", "host", "Makefile")).read()
    assert "cln" in re.search(r"^SIDE_OPEN = (.*)$", host, flags=re.M).group(1).split()
    assert "$(SIDE_OPEN:%=-lraft_hip_%) $(SIDE_LATER:%=-lraft_hip_%) " in host
    assert all(os.path.exists(os.path.join(ROOT, "include", h)) for h in ("raft_host_cln.h", "raft_hip_cln.h"))
    assert all(os.path.exists(os.path.join(ROOT, "raft_amd", "csrc", f)) for f in ("graph_clean.hpp", "graph_clean_rule.hpp", "graph_clean_lib.hip", "exports_cln.map"))
    ctx = open(os.path.join(ROOT, "raft_amd", "csrc", "engine_ctx.hpp")).read()
    assert re.search(r"^\s*DevBufSet<kClnBufs> cln\{bufs\};", ctx, flags=re.M)
    lib = open(os.path.join(ROOT, "raft_amd", "csrc", "graph_clean_lib.hip")).read()
    for helper in ("stage_host", "QueryTimer", "clear_ctl", "read_ctl", "queue_copies", "first_bad_record", "radix_sort_by_key", "utg_rank"):
        assert re.search(r"\b%s\b" % helper, lib), helper
    # the ranking is unitig.hpp's, included and not restated
    kernels = open(os.path.join(ROOT, "raft_amd", "csrc", "graph_clean.hpp")).read()
    assert '#include "unitig.hpp"' in kernels and "utg_jump_kernel" not in re.sub(r"//.*", "", kernels) and "s.next = t.next" not in kernels
    assert re.search(r"\butg_rank\(", open(os.path.join(ROOT, "raft_amd", "csrc", "unitig_lib.hip")).read())


def test_load_side_library_looks_in_the_open_table_too(monkeypatch):
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
    for tag in ("cln", "ctn", "sg", "low"):
        lib = engine.load_side_library(tag)
        assert engine.load_side_library(tag) is lib
    assert [o for o in opened if o != "libraft_hip.so"] == ["libraft_hip_cln.so", "libraft_hip_ctn.so", "libraft_hip_sg.so", "libraft_hip_low.so"]
    with pytest.raises(KeyError):
        engine.load_side_library("nope")


def _exported(file):
    path = os.path.join(os.path.dirname(engine._LIB_PATH), file)
    assert os.path.exists(path)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_cln.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    if shutil.which("nm") is not None:
        assert _exported("libraft_hip_cln.so") == ENTRY_POINTS
        assert _exported("libraft_hip_utg.so") == ["raft_hip_unitigs_device", "raft_hip_unitigs_host", "raft_hip_utg_abi"]


# ---- what Engine.graph_clean hands over: four reads, three edges
RL = np.array([100, 250, 49, 77], np.int32)
EU, EW, ES = np.array([1, 3, 5], np.int32), np.array([2, 4, 6], np.int32), np.array([40, 30, 20], np.int32)
SKIP = np.array([0, 0, 0, 0], np.uint8)
HOST = dict(rl=RL, u=EU, w=EW, s=ES, skip=SKIP)
D = {k: T(0x10000 * (i + 1), 4 if k == "rl" else 3) for i, k in enumerate(("rl", "u", "w", "s"))}
D["skip"] = T(0x80000, 4, torch.uint8)
NAMES = {**{a.ctypes.data: k for k, a in HOST.items()}, **{t.ptr: "d_" + k for k, t in D.items()}}
COLS = ("rl", "u", "w", "s")


def call(monkeypatch, *args, **kw):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("cln", side))
    res = eng.graph_clean(*args, **kw)
    assert len(side.calls) == 1 and eng._lib.lib_calls() == []
    return eng, side.calls[0], res


def check_outputs(res, args, n_reads=4, n_edges=3):
    """The ten arrays the library writes are the ones the result holds, in the header's order"""
    shapes = dict(edge_state=(n_edges,), edge_round=(n_edges,), read_state=(n_reads,), read_round=(n_reads,), flags=(n_reads,))
    for key, address in zip(ARRAYS, args[11:21]):
        assert res[key].dtype == (np.uint8 if key in shapes else np.int32) and res[key].shape == shapes.get(key, (n_reads, 2)), key
        assert (address != 0 and res[key].ctypes.data == address) or res[key].size == 0, key
    assert args[21] == ("_ClnSummary", dict.fromkeys(SUMMARY, 0)) and args[22] == ("i64", -1) and args[23] == ("f64", 0.0) and args[24] == ("i64", 0)
    assert list(res) == list(ARRAYS) + ["summary", "kernel_seconds", "launches"]
    assert res["summary"] == dict.fromkeys(SUMMARY, 0) and res["kernel_seconds"] == 0.0 and res["launches"] == 0


def test_the_host_form_and_the_defaults(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *[HOST[k] for k in COLS])
    assert name == "raft_hip_graph_clean_host" and len(args) == 25
    assert args[:8] == ["ctx", 4, "rl", 0, 3, "u", "w", "s"] and args[8:11] == [500, 4, 3]
    check_outputs(res, args)
    assert eng._lib.calls == []                                       # (no torch stream for host arrays)


def test_the_device_form_and_the_parameters(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *[D[k] for k in COLS], skip=D["skip"], min_ratio_permille=0, max_tip_reads=9, rounds=64)
    assert name == "raft_hip_graph_clean_device" and len(args) == 25
    assert args[:8] == ["ctx", 4, "d_rl", "d_skip", 3, "d_u", "d_w", "d_s"] and args[8:11] == [0, 9, 64]
    check_outputs(res, args)
    assert eng._lib.calls == [("use_torch_stream", [])] and eng.last_graph_clean_seconds == 0.0 and eng.last_graph_clean_launches == 0
    with pytest.raises(TypeError):                                    # the parameters are keyword-only, as the signature has them
        eng.graph_clean(*[HOST[k] for k in COLS], None, 5)
    _, (name, args), _ = call(monkeypatch, *[HOST[k] for k in COLS], skip=SKIP)
    assert name == "raft_hip_graph_clean_host" and args[3] == "skip"


def test_no_reads_and_no_edges(monkeypatch):
    empty = np.zeros(0, np.int32)
    _, (name, args), res = call(monkeypatch, empty, empty, empty, empty)
    assert name == "raft_hip_graph_clean_host" and args[:8] == ["ctx", 0, 0, 0, 0, 0, 0, 0]
    assert all(res[k].size == 0 for k in ARRAYS)
    _, (name, args), res = call(monkeypatch, RL, empty, empty, empty)
    assert args[:8] == ["ctx", 4, "rl", 0, 0, 0, 0, 0] and res["edge_state"].shape == (0,) and res["kept"].shape == (4, 2)


def test_what_is_refused_before_any_call(monkeypatch):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("cln", side))
    host = [HOST[k] for k in COLS]
    with pytest.raises(ValueError, match="graph_clean needs read_len, edge_u, edge_w and edge_span"):
        eng.graph_clean(*host[:3], None)
    with pytest.raises(ValueError, match="differ in length"):
        eng.graph_clean(*host[:3], ES[:2])
    with pytest.raises(ValueError, match="skip is one byte per read"):
        eng.graph_clean(*host, skip=SKIP[:3])
    dev = [D[k] for k in COLS]
    with pytest.raises(TypeError, match="skip as a contiguous uint8"):
        eng.graph_clean(*dev, skip=T(0x80000, 4, torch.int32))
    with pytest.raises(TypeError, match="contiguous int32 CUDA"):
        eng.graph_clean(*dev[:3], T(0x70000, 3, torch.int64))
    assert side.calls == [] and eng._lib.lib_calls() == []
    assert eng._ctx.value == CTX
