"""CPU: the functions of include/raft_hip_cc.h and include/raft_host_cc.h are declared by their bindings (``CC_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; the summary is nine int64; exports_cc.map names
the three entry points and nothing of the other tables, and libraft_hip_cc.so exports exactly them.  The table of the nine side
libraries is what it was and this library stands in the one beside it, under a tag of its own.  What ``Engine.components`` hands to
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

CASES = [("raft_hip_cc.h", "raft_hip_", engine), ("raft_host_cc.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_cc_abi", "raft_hip_components_device", "raft_hip_components_host"]
HOST_FUNCTIONS = ["raft_host_write_components"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI", "FLT_ABI", "END_ABI", "BEST_ABI", "UTG_ABI", "LIFT_ABI")
SUMMARY = ["n_reads", "n_records", "edge_records", "components", "singletons", "largest_reads", "largest_bases", "total_bases",
           "reads_in_largest_permille"]
RESULT = ["component", "degree", "comp_first", "comp_reads", "comp_bases", "comp_sides"]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_cc", "raft_host_cc"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.CC_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.CC_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_three_entry_points_the_summary_and_the_masks():
    assert sorted(header_functions("raft_hip_cc.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.CC_ABI)
    assert sorted(header_functions("raft_host_cc.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.CC_ABI)
    raw = open(os.path.join(ROOT, "include", "raft_hip_cc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef struct raft_hip_cc_summary \{(.*?)\}", text, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
    assert fields == [n for n, _ in engine._CcSummary._fields_] == SUMMARY
    assert all(t is C.c_int64 for _, t in engine._CcSummary._fields_) and C.sizeof(engine._CcSummary) == 72
    # the two forms take the same parameters: the context, the nine of the columns, strand, H, F, the mask, symmetric, six outputs, the
    # summary, error_index, the seconds, the launches
    dev, host = (header_functions("raft_hip_cc.h", "raft_hip_")[n] for n in ENTRY_POINTS[1:])
    assert dev == host and len(dev[1]) == 25
    # ... those of raft_hip_overlap_ends_* up to the strand, H and F; then the mask in front of symmetric
    ends = header_functions("raft_hip_end.h", "raft_hip_")["raft_hip_overlap_ends_device"][1]
    assert dev[1][:13] == ends[:13] and dev[1][13:15] == ["int32", "int32"]
    masks = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define RAFT_HIP_CC_KINDS_([A-Z]+)\s+(\d+)\b", text, flags=re.M)}
    assert masks == {"PROPER": engine.CC_KINDS_PROPER, "ALL": engine.CC_KINDS_ALL}
    kinds = [engine.END_QUERY_CONTAINED, engine.END_TARGET_CONTAINED, engine.END_QUERY_3, engine.END_QUERY_5]
    assert engine.CC_KINDS_PROPER == sum(1 << k for k in kinds) and engine.CC_KINDS_ALL == engine.CC_KINDS_PROPER | 1 << engine.END_INTERNAL


def test_the_nine_stay_and_the_library_stands_beside_them():
    assert list(engine._SIDE) == SIDE_TAGS and len(engine._SIDE) == 9
    assert engine._SIDE_LATER["cc"] == ("libraft_hip_cc.so", engine.CC_ABI, "raft_hip_cc_abi")
    assert not (set(engine._SIDE) & set(engine._SIDE_LATER))
    rows = list(engine._SIDE.values()) + list(engine._SIDE_LATER.values())
    assert all(len(row) == 3 for row in rows) and len({row[0] for row in rows}) == len(rows) == len({row[2] for row in rows})
    for tag, (file, abi, abi_fn) in engine._SIDE_LATER.items():
        assert file == f"libraft_hip_{tag}.so" and abi_fn == f"raft_hip_{tag}_abi" and abi_fn in abi
    makefile = open(os.path.join(ROOT, "raft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SIDE \+= cc=components_lib$", makefile, flags=re.M)
    assert (makefile.index("\nSIDE += utg=unitig_lib") < makefile.index("\nSIDE += lift=lift_lib") < makefile.index("\nSIDE += cc=components_lib")
            < makefile.index("\nSIDE_TAGS ="))
    host = open(os.path.join(ROOT, "raft_amd", "host", "Makefile")).read()
    assert re.search(r"^SIDE = (.*)$", host, flags=re.M).group(1).split()[:2] == ["cc", "lift"] and "$(SIDE:%=-lraft_hip_%)" in host
    assert all(os.path.exists(os.path.join(ROOT, "include", h)) for h in ("raft_host_cc.h", "raft_hip_cc.h"))


def test_load_side_library_looks_in_both_tables(monkeypatch):
    opened = []

    class Opened:
        def __init__(self, path):
            opened.append(os.path.basename(path))

        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            fn = lambda *a: 11
            return fn
    monkeypatch.setattr(engine, "_side_libs", {})
    monkeypatch.setattr(engine, "load_library", lambda: Opened("libraft_hip.so"))
    monkeypatch.setattr(engine.C, "CDLL", Opened)
    monkeypatch.setattr(engine.os.path, "exists", lambda p: True)
    for tag in ("cc", "lift", "low"):
        lib = engine.load_side_library(tag)
        assert engine.load_side_library(tag) is lib
    assert [o for o in opened if o != "libraft_hip.so"] == ["libraft_hip_cc.so", "libraft_hip_lift.so", "libraft_hip_low.so"]
    with pytest.raises(KeyError):
        engine.load_side_library("nope")


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("components" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and not any("components" in n for n in hostio.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())


def _exported(file):
    path = os.path.join(os.path.dirname(engine._LIB_PATH), file)
    assert os.path.exists(path)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_cc.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    assert os.path.exists(os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_cc.so"))
    if shutil.which("nm") is not None:
        assert _exported("libraft_hip_cc.so") == ENTRY_POINTS
        assert _exported("libraft_hip_lift.so") == ["raft_hip_lift_abi", "raft_hip_lift_overlaps_device", "raft_hip_lift_overlaps_host"]


# ---- what Engine.components hands over: three reads, four records
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
    monkeypatch.setattr(engine, "load_side_library", side_library("cc", side))
    res = eng.components(*args, **kw)
    assert len(side.calls) == 1 and eng._lib.lib_calls() == []
    return eng, side.calls[0], res


def check_outputs(res, args, n_reads=3):
    """The six arrays the library writes are the ones the result holds (the rows cut to the summary's C: the stand-in says 0)"""
    dtypes = dict(component=np.int32, degree=np.int32, comp_first=np.int32, comp_reads=np.int32, comp_bases=np.int64, comp_sides=np.int64)
    for key, address in zip(RESULT, args[15:21]):
        assert res[key].dtype == dtypes[key] and res[key].shape == ((n_reads,) if key in ("component", "degree") else (0,)), key
        assert address != 0 and (res[key].size == 0 or res[key].ctypes.data == address), key
        assert (res[key].base if res[key].base is not None else res[key]).size == n_reads, key       # sized by n_reads
    assert args[21] == ("_CcSummary", dict.fromkeys(SUMMARY, 0)) and args[22] == ("i64", -1) and args[23] == ("f64", 0.0) and args[24] == ("i64", 0)
    assert sorted(res) == sorted(RESULT + ["summary", "kernel_seconds", "launches"])
    assert res["summary"] == dict.fromkeys(SUMMARY, 0) and res["kernel_seconds"] == 0.0 and res["launches"] == 0


def test_the_host_form_and_the_defaults(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *[HOST[k] for k in COLS])
    assert name == "raft_hip_components_host" and len(args) == 25
    assert args[:11] == ["ctx", 3, "rl", 4, "qid", "qs", "qe", "tid", "ts", "te", "strand"]
    assert args[11:15] == [1000, 800, engine.CC_KINDS_PROPER, 0]
    check_outputs(res, args)
    assert eng._lib.calls == []                                       # (no torch stream for host arrays)


def test_the_device_form_and_the_parameters(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *[D[k] for k in COLS], max_overhang=7, min_ratio_permille=900, kind_mask=engine.CC_KINDS_ALL,
                                  symmetric=True)
    assert name == "raft_hip_components_device" and len(args) == 25
    assert args[:11] == ["ctx", 3, "d_rl", 4, "d_qid", "d_qs", "d_qe", "d_tid", "d_ts", "d_te", "d_strand"]
    assert args[11:15] == [7, 900, 62, 1]
    check_outputs(res, args)
    assert eng._lib.calls == [("use_torch_stream", [])]
    assert eng.last_components_launches == 0 and eng.last_components_seconds == 0.0
    # positional, as the signature of the issue has them
    _, (_, args), _ = call(monkeypatch, *[HOST[k] for k in COLS], 5, 6, 4, True)
    assert args[11:15] == [5, 6, 4, 1]


def test_the_rows_are_cut_to_the_summary(monkeypatch):
    eng = make_engine(NAMES)

    class Two(Lib):
        def __getattr__(self, name):
            fn = super().__getattr__(name)

            def wrapped(*args):
                rc = fn(*args)
                args[21]._obj.components = 2
                return rc
            return wrapped
    monkeypatch.setattr(engine, "load_side_library", side_library("cc", Two(NAMES)))
    res = eng.components(*[HOST[k] for k in COLS])
    assert all(res[k].shape == (2,) for k in RESULT[2:]) and all(res[k].shape == (3,) for k in RESULT[:2]) and res["summary"]["components"] == 2


def test_no_reads_and_no_records(monkeypatch):
    empty, none = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    _, (name, args), res = call(monkeypatch, empty, *[empty] * 6, none)
    assert name == "raft_hip_components_host" and args[:11] == ["ctx", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert all(res[k].shape == (0,) for k in RESULT)


def test_what_is_refused_before_any_call(monkeypatch):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("cc", side))
    host = [HOST[k] for k in COLS]
    with pytest.raises(ValueError, match="components needs read_len, the six columns and strand"):
        eng.components(*host[:7], None)
    with pytest.raises(ValueError, match="components needs"):
        eng.components(*host[:5], None, *host[6:])
    with pytest.raises(ValueError, match="differ in length"):
        eng.components(*host[:7], STRAND[:3])
    dev = [D[k] for k in COLS]
    with pytest.raises(TypeError, match="strand as a contiguous uint8"):
        eng.components(*dev[:7], T(0x80000, 4, torch.int32))
    with pytest.raises(TypeError, match="contiguous int32 CUDA"):
        eng.components(*dev[:6], T(0x70000, 4, torch.int64), dev[7])
    assert side.calls == [] and eng._lib.lib_calls() == []
    assert eng._ctx.value == CTX
