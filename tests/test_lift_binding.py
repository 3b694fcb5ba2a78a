"""CPU: the functions of include/raft_hip_lift.h and include/raft_host_lift.h are declared by their bindings (``LIFT_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; the summary is six int64; exports_lift.map names
the three entry points and nothing of the other tables, and libraft_hip_lift.so exports exactly them.  The library is registered
under its tag in the one table of side libraries.  What ``Engine.lift_overlaps`` hands to the library, against the recording stand-in of
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
from raft_testlib import ROOT
from test_binding_calls import CTX, Lib, T, check_side_table, make_engine, side_library
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_lift.h", "raft_hip_", engine), ("raft_host_lift.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_lift_abi", "raft_hip_lift_overlaps_device", "raft_hip_lift_overlaps_host"]
HOST_FUNCTIONS = ["raft_host_write_fragment_paf"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI", "FLT_ABI", "END_ABI", "BEST_ABI", "UTG_ABI")
SUMMARY = ["n_records", "n_out", "records_none", "records_cut", "pairs_dropped", "most_per_record"]
COLUMNS = ["qfrag", "qs", "qe", "tfrag", "ts", "te", "rev", "src"]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_lift", "raft_host_lift"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.LIFT_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.LIFT_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_three_entry_points_and_the_summary():
    assert sorted(header_functions("raft_hip_lift.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.LIFT_ABI)
    assert sorted(header_functions("raft_host_lift.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.LIFT_ABI)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raft_hip_lift.h")).read(), flags=re.S)
    body = re.search(r"typedef struct raft_hip_lift_summary \{(.*?)\}", text, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
    assert fields == [n for n, _ in engine._LiftSummary._fields_] == SUMMARY
    assert all(t is C.c_int64 for _, t in engine._LiftSummary._fields_) and C.sizeof(engine._LiftSummary) == 48
    # the two forms take the same parameters: the context, n_reads, the records, strand, the table, min_len, out_cap, eight outputs,
    # the summary, error_index, the seconds
    dev, host = (header_functions("raft_hip_lift.h", "raft_hip_")[n] for n in ENTRY_POINTS[1:])
    assert dev == host and len(dev[1]) == 18
    assert tuple(COLUMNS) == engine.LIFT_COLUMNS


def test_the_library_is_registered_under_its_tag():
    check_side_table("lift", engine.LIFT_ABI)
    makefile = open(os.path.join(ROOT, "raft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SIDE \+= lift=lift_lib$", makefile, flags=re.M)
    assert makefile.index("\nSIDE += utg=unitig_lib") < makefile.index("\nSIDE += lift=lift_lib") < makefile.index("\nSIDE_TAGS =")
    host = open(os.path.join(ROOT, "raft_amd", "host", "Makefile")).read()
    # (the CLI links every library of the SIDE list, and both host targets depend on every public header)
    assert "lift" in re.search(r"^SIDE = (.*)$", host, flags=re.M).group(1).split() and "$(SIDE:%=-lraft_hip_%)" in host
    assert "HDRS = $(wildcard ../../include/*.h)" in host and host.count(" $(HDRS)") == 2
    assert all(os.path.exists(os.path.join(ROOT, "include", h)) for h in ("raft_host_lift.h", "raft_hip_lift.h"))


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("lift" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and not any("fragment_paf" in n for n in hostio.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())
    check_side_table("utg", engine.UTG_ABI)
    assert sorted(header_functions("raft_hip_utg.h", "raft_hip_")) == sorted(engine.UTG_ABI) and len(engine.UTG_ABI) == 3


def _exported(file):
    path = os.path.join(os.path.dirname(engine._LIB_PATH), file)
    assert os.path.exists(path)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_lift.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    assert _exported("libraft_hip_lift.so") == ENTRY_POINTS
    assert _exported("libraft_hip_utg.so") == ["raft_hip_unitigs_device", "raft_hip_unitigs_host", "raft_hip_utg_abi"]


# ---- what Engine.lift_overlaps hands over: three reads, four records
QID, QS, QE = np.array([0, 1, 1, 2], np.int32), np.array([0, 10, 20, 0], np.int32), np.array([90, 200, 240, 49], np.int32)
TID, TS, TE = np.array([1, 0, 2, 1], np.int32), np.array([5, 0, 1, 2], np.int32), np.array([95, 99, 40, 50], np.int32)
STRAND = np.array([0, 1, 0, 1], np.uint8)
OFF, FB, FE = np.array([0, 1, 3, 4], np.int64), np.array([0, 0, 120, 0], np.int32), np.array([100, 130, 250, 49], np.int32)
HOST = dict(qid=QID, qs=QS, qe=QE, tid=TID, ts=TS, te=TE, strand=STRAND, off=OFF, fb=FB, fe=FE)
D = {k: T(0x10000 * (i + 1), 4) for i, k in enumerate(("qid", "qs", "qe", "tid", "ts", "te"))}
D["strand"] = T(0x70000, 4, torch.uint8)
D["off"], D["fb"], D["fe"] = T(0x80000, 4, torch.int64), T(0x90000, 4), T(0xA0000, 4)
NAMES = {**{a.ctypes.data: k for k, a in HOST.items()}, **{t.ptr: "d_" + k for k, t in D.items()}}
COLS = ("qid", "qs", "qe", "tid", "ts", "te")


def call(monkeypatch, *args, **kw):
    eng = make_engine(NAMES, n_reads=3)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("lift", side))
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: real_empty(*a, **k))          # (no device on this machine)
    res = eng.lift_overlaps(*args, **kw)
    assert eng._lib.lib_calls() == []
    return eng, side.calls, res


def check_result(res, tensors):
    assert sorted(res) == sorted(COLUMNS + SUMMARY + ["kernel_seconds"])
    for k in COLUMNS:
        want = (torch.uint8 if k == "rev" else torch.int32) if tensors else (np.uint8 if k == "rev" else np.int32)
        assert res[k].dtype == want and tuple(res[k].shape) == (0,), k
    assert all(res[k] == 0 for k in SUMMARY) and res["kernel_seconds"] == 0.0


def test_the_host_form(monkeypatch):
    eng, calls, res = call(monkeypatch, *[HOST[k] for k in COLS], STRAND, fragments=(OFF, FB, FE), min_len=7)
    # the size query (the stand-in answers n_out = 0, so the filling call is not made)
    assert len(calls) == 1
    name, args = calls[0]
    assert name == "raft_hip_lift_overlaps_host" and len(args) == 18
    assert args[0] == "ctx" and args[1] == 3
    assert args[2] == ("_Records", dict(n_rec=4, d_qid="qid", d_qs="qs", d_qe="qe", d_tid="tid", d_ts="ts", d_te="te"))
    assert args[3] == "strand" and args[4] == ("_FragTable", dict(n=4, offset="off", first="fb", second="fe"))
    assert args[5:7] == [7, 0] and args[7:15] == [0] * 8
    assert args[15] == ("_LiftSummary", dict.fromkeys(SUMMARY, 0)) and args[16] == ("i64", -1) and args[17] == ("f64", 0.0)
    check_result(res, False)
    assert eng._lib.calls == []                                       # (no torch stream for host arrays)


def test_the_own_pass_and_the_default_min_len(monkeypatch):
    _, calls, res = call(monkeypatch, *[HOST[k] for k in COLS], STRAND)
    name, args = calls[0]
    assert name == "raft_hip_lift_overlaps_host" and args[1] == 3      # n_reads: the finished pass's
    assert args[4] == ("_FragTable", dict(n=-1, offset=0, first=0, second=0)) and args[5:7] == [1, 0]
    check_result(res, False)


def test_the_device_form(monkeypatch):
    eng, calls, res = call(monkeypatch, *[D[k] for k in COLS], D["strand"], fragments=(D["off"], D["fb"], D["fe"]))
    assert len(calls) == 1
    name, args = calls[0]
    assert name == "raft_hip_lift_overlaps_device" and args[1] == 3
    assert args[2] == ("_Records", dict(n_rec=4, d_qid="d_qid", d_qs="d_qs", d_qe="d_qe", d_tid="d_tid", d_ts="d_ts", d_te="d_te"))
    assert args[3] == "d_strand" and args[4] == ("_FragTable", dict(n=4, offset="d_off", first="d_fb", second="d_fe")) and args[7:15] == [0] * 8
    check_result(res, True)
    assert eng._lib.calls == [("use_torch_stream", [])]
    assert eng.last_lift_overlaps_seconds == 0.0


def test_the_filling_call(monkeypatch):
    """When the size query answers n_out = 5, the second call hands over eight arrays of five elements and that capacity."""
    eng = make_engine(NAMES, n_reads=3)

    class Five(Lib):
        def __getattr__(self, name):
            fn = super().__getattr__(name)

            def wrapped(*args):
                rc = fn(*args)
                args[15]._obj.n_out = 5
                return rc
            return wrapped
    side = Five(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("lift", side))
    res = eng.lift_overlaps(*[HOST[k] for k in COLS], STRAND, fragments=(OFF, FB, FE))
    assert [c[0] for c in side.calls] == ["raft_hip_lift_overlaps_host"] * 2
    first, second = side.calls[0][1], side.calls[1][1]
    assert first[6] == 0 and first[7:15] == [0] * 8 and second[6] == 5 and second[:6] == first[:6]
    assert second[7:15] == [res[k].ctypes.data for k in COLUMNS] and all(res[k].shape == (5,) for k in COLUMNS)
    assert res["n_out"] == 5


def test_what_is_refused_before_any_call(monkeypatch):
    eng = make_engine(NAMES, n_reads=3)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("lift", side))
    cols = [HOST[k] for k in COLS]
    with pytest.raises(ValueError, match="the six columns and strand"):
        eng.lift_overlaps(*cols, None)
    with pytest.raises(ValueError, match="the six columns and strand"):
        eng.lift_overlaps(*cols[:5], None, STRAND)
    with pytest.raises(ValueError, match="fragments is"):
        eng.lift_overlaps(*cols, STRAND, fragments=(OFF, FB))
    with pytest.raises(ValueError, match="two arrays of one length"):
        eng.lift_overlaps(*cols, STRAND, fragments=(OFF, FB, FE[:3]))
    with pytest.raises(ValueError, match="differ in length"):
        eng.lift_overlaps(*cols, STRAND[:3], fragments=(OFF, FB, FE))
    dev = [D[k] for k in COLS]
    with pytest.raises(TypeError, match="strand as a contiguous uint8"):
        eng.lift_overlaps(*dev, T(0x70000, 4, torch.int32), fragments=(D["off"], D["fb"], D["fe"]))
    with pytest.raises(TypeError, match="frag_offset as a contiguous int64"):
        eng.lift_overlaps(*dev, D["strand"], fragments=(T(0x80000, 4, torch.int32), D["fb"], D["fe"]))
    with pytest.raises(TypeError, match="contiguous int32 CUDA"):
        eng.lift_overlaps(*dev[:5], T(0x60000, 4, torch.int64), D["strand"], fragments=(D["off"], D["fb"], D["fe"]))
    assert side.calls == [] and eng._lib.lib_calls() == []
    assert eng._ctx.value == CTX
