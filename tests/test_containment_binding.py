"""CPU: the functions of include/raft_hip_ctn.h and include/raft_host_ctn.h are declared by their bindings (``CTN_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; the summaries are eleven and six int64;
exports_ctn.map names the five entry points and nothing of the other tables, and libraft_hip_ctn.so exports exactly them.  The two
closed tables of side libraries are what they were and this library stands in a third, which ``load_side_library`` looks through as
well.  What ``Engine.containment`` and ``Engine.place_contained`` hand to the library, against the recording stand-in of
tests/test_binding_calls.py."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from ctn_testlib import PER_READ, PLACE_PER_READ, PLACE_PER_UNITIG, PLACE_SUMMARY, SUMMARY
from raft_testlib import ROOT
from test_binding_calls import CTX, SIDE_TAGS, Lib, T, make_engine, side_library
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_ctn.h", "raft_hip_", engine), ("raft_host_ctn.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_containment_device", "raft_hip_containment_host", "raft_hip_ctn_abi", "raft_hip_place_contained_device",
                "raft_hip_place_contained_host"]
HOST_FUNCTIONS = ["raft_host_write_containment", "raft_host_write_unitig_depth"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI", "FLT_ABI", "END_ABI", "BEST_ABI", "UTG_ABI", "LIFT_ABI", "CC_ABI", "SG_ABI")


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_ctn", "raft_host_ctn"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.CTN_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.CTN_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_entry_points_the_summaries_and_the_flags():
    assert sorted(header_functions("raft_hip_ctn.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.CTN_ABI)
    assert sorted(header_functions("raft_host_ctn.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.CTN_ABI)
    raw = open(os.path.join(ROOT, "include", "raft_hip_ctn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for struct, cls, names in (("raft_hip_ctn_summary", engine._CtnSummary, SUMMARY), ("raft_hip_place_summary", engine._PlaceSummary, PLACE_SUMMARY)):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, text, flags=re.S).group(1)
        assert re.findall(r"\b([a-z0-9_]+)\s*[,;]", body) == [n for n, _ in cls._fields_] == names
        assert all(t is C.c_int64 for _, t in cls._fields_) and C.sizeof(cls) == 8 * len(names)
    fns = header_functions("raft_hip_ctn.h", "raft_hip_")
    dev, host = fns["raft_hip_containment_device"], fns["raft_hip_containment_host"]
    assert dev == host and len(dev[1]) == 28
    # ... those of raft_hip_overlap_ends_* up to symmetric: the context, the nine of the columns, strand, H, F, symmetric
    ends = header_functions("raft_hip_end.h", "raft_hip_")["raft_hip_overlap_ends_device"][1]
    assert dev[1][:14] == ends[:14]
    dev, host = fns["raft_hip_place_contained_device"], fns["raft_hip_place_contained_host"]
    assert dev == host and len(dev[1]) == 20
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define RAFT_HIP_CTN_([A-Z_]+)\s+(\d+)\b", text, flags=re.M)}
    assert flags == {"HAS_PARENT": engine.CTN_HAS_PARENT, "PARENT_REV": engine.CTN_PARENT_REV, "ROOT_REV": engine.CTN_ROOT_REV,
                     "UNPLACED_VIEW": engine.CTN_UNPLACED_VIEW, "ORPHAN": engine.CTN_ORPHAN, "MAX_READS": engine.CTN_MAX_READS}
    assert engine.CTN_MAX_READS == 2 ** 30 - 1 == engine.UTG_MAX_READS
    assert dict(engine.CTN_PER_READ) == PER_READ and dict(engine.PLACE_PER_READ) == PLACE_PER_READ and dict(engine.PLACE_PER_UNITIG) == PLACE_PER_UNITIG


def test_the_closed_tables_stay_and_the_library_stands_in_a_third():
    assert list(engine._SIDE) == SIDE_TAGS and len(engine._SIDE) == 9 and list(engine._SIDE_LATER) == ["cc", "sg"]
    assert engine._SIDE_THIRD["ctn"] == ("libraft_hip_ctn.so", engine.CTN_ABI, "raft_hip_ctn_abi")
    assert engine._SIDE_TABLES == (engine._SIDE, engine._SIDE_LATER, engine._SIDE_THIRD)
    tags = [t for table in engine._SIDE_TABLES for t in table]
    assert len(tags) == len(set(tags)) == 12
    rows = [row for table in engine._SIDE_TABLES for row in table.values()]
    assert all(len(row) == 3 for row in rows) and len({row[0] for row in rows}) == len(rows) == len({row[2] for row in rows})
    for tag, (file, abi, abi_fn) in engine._SIDE_THIRD.items():
        assert file == f"libraft_hip_{tag}.so" and abi_fn == f"raft_hip_{tag}_abi" and abi_fn in abi
    makefile = open(os.path.join(ROOT, "raft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SIDE \+= ctn=containment_lib$", makefile, flags=re.M)
    assert makefile.index("\nSIDE += sg=string_graph_lib") < makefile.index("\nSIDE += ctn=containment_lib") < makefile.index("\nSIDE_TAGS =")
    host = open(os.path.join(ROOT, "raft_amd", "host", "Makefile")).read()
    assert len(re.search(r"^SIDE = (.*)$", host, flags=re.M).group(1).split()) == 11 and re.search(r"^SIDE_LATER = ctn$", host, flags=re.M)
    assert "$(SIDE_LATER:%=-lraft_hip_%) $(SIDE:%=-lraft_hip_%) -lraft_hip " in host
    assert all(os.path.exists(os.path.join(ROOT, "include", h)) for h in ("raft_host_ctn.h", "raft_hip_ctn.h"))
    assert all(os.path.exists(os.path.join(ROOT, "raft_amd", "csrc", f)) for f in ("containment.hpp", "containment_rule.hpp", "containment_lib.hip", "exports_ctn.map"))
    ctx = open(os.path.join(ROOT, "raft_amd", "csrc", "engine_ctx.hpp")).read()
    assert re.search(r"^\s*DevBufSet<kCtnBufs> ctn\{bufs\};", ctx, flags=re.M)
    lib = open(os.path.join(ROOT, "raft_amd", "csrc", "containment_lib.hip")).read()
    for helper in ("check_ends_rule_call", "stage_host", "stage_columns", "QueryTimer", "clear_ctl", "read_ctl", "queue_copies", "first_bad_record"):
        assert re.search(r"\b%s\b" % helper, lib), helper


def test_load_side_library_looks_in_every_table(monkeypatch):
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
    for tag in ("ctn", "sg", "cc", "low"):
        lib = engine.load_side_library(tag)
        assert engine.load_side_library(tag) is lib
    assert [o for o in opened if o != "libraft_hip.so"] == ["libraft_hip_ctn.so", "libraft_hip_sg.so", "libraft_hip_cc.so", "libraft_hip_low.so"]
    with pytest.raises(KeyError):
        engine.load_side_library("nope")


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("contain" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and not any("contain" in n for n in hostio.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())


def _exported(file):
    path = os.path.join(os.path.dirname(engine._LIB_PATH), file)
    assert os.path.exists(path)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_ctn.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    assert os.path.exists(os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_ctn.so"))
    if shutil.which("nm") is not None:
        assert _exported("libraft_hip_ctn.so") == ENTRY_POINTS
        assert _exported("libraft_hip_sg.so") == ["raft_hip_sg_abi", "raft_hip_string_graph_device", "raft_hip_string_graph_host"]


# ---- what Engine.containment hands over: three reads, four records
RL = np.array([100, 250, 49], np.int32)
QID, QS, QE = np.array([0, 1, 1, 2], np.int32), np.array([0, 10, 20, 0], np.int32), np.array([90, 200, 240, 49], np.int32)
TID, TS, TE = np.array([1, 0, 2, 1], np.int32), np.array([5, 0, 1, 2], np.int32), np.array([95, 99, 40, 50], np.int32)
STRAND = np.array([0, 1, 0, 1], np.uint8)
HOST = dict(rl=RL, qid=QID, qs=QS, qe=QE, tid=TID, ts=TS, te=TE, strand=STRAND)
D = {k: T(0x10000 * (i + 1), 3 if k == "rl" else 4) for i, k in enumerate(("rl", "qid", "qs", "qe", "tid", "ts", "te"))}
D["strand"] = T(0x80000, 4, torch.uint8)
NAMES = {**{a.ctypes.data: k for k, a in HOST.items()}, **{t.ptr: "d_" + k for k, t in D.items()}}
COLS = ("rl", "qid", "qs", "qe", "tid", "ts", "te", "strand")


def call(monkeypatch, *args, **kw):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("ctn", side))
    res = eng.containment(*args, **kw)
    assert len(side.calls) == 1 and eng._lib.lib_calls() == []
    return eng, side.calls[0], res


def check_outputs(res, args, n_reads=3):
    """The eleven arrays the library writes are the ones the result holds"""
    for (key, dt), address in zip(PER_READ.items(), args[14:25]):
        assert res[key].dtype == dt and res[key].shape == (n_reads,), key
        assert address != 0 and res[key].ctypes.data == address, key
    assert args[25] == ("_CtnSummary", dict.fromkeys(SUMMARY, 0)) and args[26] == ("i64", -1) and args[27] == ("f64", 0.0)
    assert list(res) == list(PER_READ) + ["summary", "kernel_seconds"]
    assert res["summary"] == dict.fromkeys(SUMMARY, 0) and res["kernel_seconds"] == 0.0


def test_the_host_form_and_the_defaults(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *[HOST[k] for k in COLS])
    assert name == "raft_hip_containment_host" and len(args) == 28
    assert args[:11] == ["ctx", 3, "rl", 4, "qid", "qs", "qe", "tid", "ts", "te", "strand"]
    assert args[11:14] == [1000, 800, 0]
    check_outputs(res, args)
    assert eng._lib.calls == []                                       # (no torch stream for host arrays)


def test_the_device_form_and_the_parameters(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *[D[k] for k in COLS], max_overhang=7, min_ratio_permille=900, symmetric=True)
    assert name == "raft_hip_containment_device" and len(args) == 28
    assert args[:11] == ["ctx", 3, "d_rl", 4, "d_qid", "d_qs", "d_qe", "d_tid", "d_ts", "d_te", "d_strand"]
    assert args[11:14] == [7, 900, 1]
    check_outputs(res, args)
    assert eng._lib.calls == [("use_torch_stream", [])] and eng.last_containment_seconds == 0.0
    with pytest.raises(TypeError):                                    # the parameters are keyword-only, as the signature has them
        eng.containment(*[HOST[k] for k in COLS], 5)


def test_no_reads_and_no_records(monkeypatch):
    empty, none = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    _, (name, args), res = call(monkeypatch, empty, *[empty] * 6, none)
    assert name == "raft_hip_containment_host" and args[:11] == ["ctx", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert all(res[k].shape == (0,) for k in PER_READ)


def test_what_is_refused_before_any_call(monkeypatch):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("ctn", side))
    host = [HOST[k] for k in COLS]
    with pytest.raises(ValueError, match="containment needs read_len, the six columns and strand"):
        eng.containment(*host[:7], None)
    with pytest.raises(ValueError, match="containment needs"):
        eng.containment(*host[:5], None, *host[6:])
    with pytest.raises(ValueError, match="differ in length"):
        eng.containment(*host[:7], STRAND[:3])
    dev = [D[k] for k in COLS]
    with pytest.raises(TypeError, match="strand as a contiguous uint8"):
        eng.containment(*dev[:7], T(0x80000, 4, torch.int32))
    with pytest.raises(TypeError, match="contiguous int32 CUDA"):
        eng.containment(*dev[:6], T(0x70000, 4, torch.int64), dev[7])
    assert side.calls == [] and eng._lib.lib_calls() == []
    assert eng._ctx.value == CTX


# ---- what Engine.place_contained hands over: three reads, two unitigs
P_HOST = dict(rl=RL, root=np.array([0, 0, 2], np.int32), root_pos=np.array([0, 7, 0], np.int32), flags=np.array([0, 5, 0], np.uint8),
              unitig=np.array([0, -1, 1], np.int32), offset=np.array([0, 0, 0], np.int64), orient=np.array([0, 0, 1], np.uint8),
              utg_length=np.array([100, 49], np.int64))
P_DTYPES = dict(rl=torch.int32, root=torch.int32, root_pos=torch.int32, flags=torch.uint8, unitig=torch.int32, offset=torch.int64, orient=torch.uint8,
                utg_length=torch.int64)
P_D = {k: T(0x100000 * (i + 1), 2 if k == "utg_length" else 3, dt) for i, (k, dt) in enumerate(P_DTYPES.items())}
P_NAMES = {**{a.ctypes.data: k for k, a in P_HOST.items()}, **{t.ptr: "d_" + k for k, t in P_D.items()}}
P_ORDER = ("rl", "root", "root_pos", "flags", "unitig", "offset", "orient")


def place(monkeypatch, src, **change):
    eng = make_engine(P_NAMES)
    side = Lib(P_NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("ctn", side))
    a = dict(src, **change)
    res = eng.place_contained(a["rl"], dict(root=a["root"], root_pos=a["root_pos"], flags=a["flags"], depth="not looked at"), a["unitig"], a["offset"],
                              a["orient"], a["utg_length"])
    assert len(side.calls) == 1 and eng._lib.lib_calls() == []
    return eng, side.calls[0], res


@pytest.mark.parametrize("form", ["host", "device"])
def test_place_contained_hands_over_the_forest_and_the_layout(monkeypatch, form):
    eng, (name, args), res = place(monkeypatch, P_HOST if form == "host" else P_D)
    pre = "" if form == "host" else "d_"
    assert name == f"raft_hip_place_contained_{form}" and len(args) == 20
    assert args[:11] == ["ctx", 3] + [pre + k for k in P_ORDER] + [2, pre + "utg_length"]
    table = {**PLACE_PER_READ, **PLACE_PER_UNITIG}
    for (key, dt), address in zip(table.items(), args[11:17]):
        assert res[key].dtype == dt and res[key].shape == ((3,) if key in PLACE_PER_READ else (2,)) and res[key].ctypes.data == address, key
    assert args[17] == ("_PlaceSummary", dict.fromkeys(PLACE_SUMMARY, 0)) and args[18] == ("i64", -1) and args[19] == ("f64", 0.0)
    assert list(res) == list(table) + ["summary", "kernel_seconds"] and res["summary"] == dict.fromkeys(PLACE_SUMMARY, 0)
    assert eng._lib.calls == ([] if form == "host" else [("use_torch_stream", [])]) and eng.last_place_contained_seconds == 0.0


def test_place_contained_refuses_before_any_call(monkeypatch):
    with pytest.raises(ValueError, match="one value per read"):
        place(monkeypatch, P_HOST, unitig=P_HOST["unitig"][:2])
    with pytest.raises(ValueError, match="place_contained needs"):
        place(monkeypatch, P_HOST, offset=None)
    with pytest.raises(TypeError, match="place_contained needs contiguous CUDA tensors"):
        place(monkeypatch, P_D, offset=T(0x600000, 3, torch.int32))
    with pytest.raises(KeyError):
        make_engine(P_NAMES).place_contained(RL, dict(root=P_HOST["root"]), *[P_HOST[k] for k in ("unitig", "offset", "orient", "utg_length")])
