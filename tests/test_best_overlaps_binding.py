"""CPU: the functions of include/raft_hip_best.h and include/raft_host_best.h are declared by their bindings (``BEST_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; the summary is nine int64; exports_best.map names
the three entry points and nothing of the other tables, and libraft_hip_best.so exports exactly them.  The closed sets -- raft_hip.h,
raft_host.h, raft_host_flt.h, raft_host_end.h, libraft_hip_end.so, the tags of ``engine._SIDE`` -- are what they were.  What
``Engine.best_overlaps`` hands to the library, against the recording stand-in of tests/test_binding_calls.py."""
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
from test_binding_calls import CTX, D, DEV_NAMES, HOST_NAMES, QE, QID, QS, RL, TE, TID, TS, Lib, T, check_side_table, make_engine, side_library
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_best.h", "raft_hip_", engine), ("raft_host_best.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_best_abi", "raft_hip_best_overlaps_device", "raft_hip_best_overlaps_host"]
HOST_FUNCTIONS = ["raft_host_write_best_overlaps"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI", "FLT_ABI", "END_ABI")
SUMMARY = ["n_records", "candidates", "left_out", "ends_best", "ends_mutual", "reads_both_best", "reads_both_mutual", "reads_no_best", "reads_skipped"]


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_best", "raft_host_best"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.BEST_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.BEST_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_three_entry_points_and_the_summary():
    assert sorted(header_functions("raft_hip_best.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.BEST_ABI)
    assert sorted(header_functions("raft_host_best.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.BEST_ABI)
    text = _header("raft_hip_best.h")
    body = re.search(r"typedef struct raft_hip_best_summary \{(.*?)\}", text, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
    assert fields == [n for n, _ in engine._BestSummary._fields_] == SUMMARY
    assert all(t is C.c_int64 for _, t in engine._BestSummary._fields_) and re.findall(r"\b(\w+)\s+[a-z0-9_]+\s*;", body) == ["int64_t"] * 9
    assert C.sizeof(engine._BestSummary) == 72
    # the two forms take the same parameters: the context, n_reads, read_len, n_rec, six columns, strand, skip, H, F, symmetric,
    # partner, span, flags, the summary, error_index, the seconds
    dev, host = (header_functions("raft_hip_best.h", "raft_hip_")[n] for n in ENTRY_POINTS[1:])
    assert dev == host and len(dev[1]) == 21
    bits = {k: int(v) for k, v in re.findall(r"#define RAFT_HIP_BEST_([A-Z0-9]+) (\d+)", text)}
    assert bits == {"REV5": engine.BEST_REV5, "MUTUAL5": engine.BEST_MUTUAL5, "REV3": engine.BEST_REV3, "MUTUAL3": engine.BEST_MUTUAL3,
                    "SKIPPED": engine.BEST_SKIPPED} == {"REV5": 1, "MUTUAL5": 2, "REV3": 4, "MUTUAL3": 8, "SKIPPED": 16}


def test_the_rule_header_states_the_same_numbers():
    """raft_amd/csrc/best_ovl_rule.hpp, which the kernels use, packs the key and numbers the flag bits as the public header does."""
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "best_ovl_rule.hpp")).read()
    got = {n: int(v) for n, v in re.findall(r"\bkBest([A-Za-z0-9]+) = (\d+)", text)}
    assert (got["SpanShift"], got["PartnerShift"], got["RevShift"]) == (33, 2, 1) and "kBestPartnerMask = 0x7FFFFFFFull" in text
    assert [got[n] for n in ("Rev5", "Mutual5", "Rev3", "Mutual3", "Skipped")] == [1, 2, 4, 8, 16]
    assert "(uint64)span << 33 | (uint64)(0x7FFFFFFF - other) << 2 | (uint64)rev << 1" in open(os.path.join(ROOT, "include", "raft_hip_best.h")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["cstdint", "ovl_ends_rule.hpp"]


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("best" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and not any("best" in n for n in hostio.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())
    assert "best" not in open(os.path.join(ROOT, "include", "raft_host.h")).read()
    assert sorted(header_functions("raft_host_flt.h", "raft_host_")) == sorted(hostio.FLT_ABI) and len(hostio.FLT_ABI) == 3
    assert sorted(header_functions("raft_host_end.h", "raft_host_")) == sorted(hostio.END_ABI) and len(hostio.END_ABI) == 4
    assert sorted(header_functions("raft_hip_end.h", "raft_hip_")) == sorted(engine.END_ABI) and len(engine.END_ABI) == 3
    # the library stands under its tag in the one table, which holds the nine libraries and no other
    check_side_table("best", engine.BEST_ABI)
    makefile = open(os.path.join(ROOT, "raft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SIDE = .*\bend=ovl_ends_lib best=best_ovl_lib$", makefile, flags=re.M)


def _exported(file):
    path = os.path.join(os.path.dirname(engine._LIB_PATH), file)
    assert os.path.exists(path)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_best.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    assert os.path.exists(os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_best.so"))
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    assert _exported("libraft_hip_best.so") == ENTRY_POINTS
    assert _exported("libraft_hip_end.so") == ["raft_hip_end_abi", "raft_hip_overlap_ends_device", "raft_hip_overlap_ends_host"]


# ---- what Engine.best_overlaps hands over
STRAND, SKIP = np.array([0, 1, 0, 1], np.uint8), np.array([0, 0, 1], np.uint8)
D_STRAND, D_SKIP = T(0xB0000, 4, torch.uint8), T(0xC0000, 3, torch.uint8)
NAMES = {**HOST_NAMES, **DEV_NAMES, STRAND.ctypes.data: "strand", SKIP.ctypes.data: "skip", D_STRAND.ptr: "d_strand", D_SKIP.ptr: "d_skip"}
HOST_COLS = (RL, QID, QS, QE, TID, TS, TE)
DEV_COLS = tuple(D[k] for k in ("rl", "qid", "qs", "qe", "tid", "ts", "te"))


def call(monkeypatch, *args, **kw):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("best", side))
    res = eng.best_overlaps(*args, **kw)
    assert len(side.calls) == 1 and eng._lib.lib_calls() == []
    return eng, side.calls[0], res


def check_outputs(res, args, n_reads=3):
    partner, span, flags = args[15:18]
    assert res["partner"].dtype == np.int32 and res["partner"].shape == (n_reads, 2) and res["partner"].ctypes.data == partner
    assert res["span"].dtype == np.int32 and res["span"].shape == (n_reads, 2) and res["span"].ctypes.data == span
    assert res["flags"].dtype == np.uint8 and res["flags"].shape == (n_reads,) and res["flags"].ctypes.data == flags
    assert args[18] == ("_BestSummary", dict.fromkeys(SUMMARY, 0)) and args[19] == ("i64", -1) and args[20] == ("f64", 0.0)
    assert sorted(res) == sorted(SUMMARY + ["partner", "span", "flags", "kernel_seconds"]) and res["kernel_seconds"] == 0.0


def test_the_host_form(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *HOST_COLS, STRAND, skip=SKIP)
    assert name == "raft_hip_best_overlaps_host" and len(args) == 21
    assert args[:15] == ["ctx", 3, "rl", 4, "qid", "qs", "qe", "tid", "ts", "te", "strand", "skip", 1000, 800, 0]
    check_outputs(res, args)
    assert eng._lib.calls == []                                       # (no torch stream for host arrays)
    _, (name, args), res = call(monkeypatch, *HOST_COLS, STRAND, max_overhang=7, min_ratio_permille=0, symmetric=True)
    assert name == "raft_hip_best_overlaps_host" and args[10:15] == ["strand", 0, 7, 0, 1]      # skip=None is NULL
    check_outputs(res, args)


def test_the_device_form(monkeypatch):
    eng, (name, args), res = call(monkeypatch, *DEV_COLS, D_STRAND, skip=D_SKIP, max_overhang=0, min_ratio_permille=1000)
    assert name == "raft_hip_best_overlaps_device"
    assert args[:15] == ["ctx", 3, "d_rl", 4, "d_qid", "d_qs", "d_qe", "d_tid", "d_ts", "d_te", "d_strand", "d_skip", 0, 1000, 0]
    check_outputs(res, args)
    assert eng._lib.calls == [("use_torch_stream", [])]
    _, (name, args), _ = call(monkeypatch, *DEV_COLS, D_STRAND)
    assert name == "raft_hip_best_overlaps_device" and args[10:12] == ["d_strand", 0]


def test_no_records_and_no_reads(monkeypatch):
    empty = np.zeros(0, np.int32)
    _, (name, args), res = call(monkeypatch, RL, *[empty] * 6, np.zeros(0, np.uint8))
    assert args[:12] == ["ctx", 3, "rl", 0, 0, 0, 0, 0, 0, 0, 0, 0]
    check_outputs(res, args)
    _, (name, args), res = call(monkeypatch, empty, *[empty] * 6, np.zeros(0, np.uint8), skip=np.zeros(0, np.uint8))
    assert args[:12] == ["ctx", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0] and args[15:18] == [0, 0, 0]
    assert res["partner"].shape == (0, 2) and res["flags"].shape == (0,)


def test_what_is_refused_before_any_call(monkeypatch):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("best", side))
    with pytest.raises(ValueError, match="best_overlaps needs read_len, the six columns and strand"):
        eng.best_overlaps(*HOST_COLS, None)
    with pytest.raises(ValueError, match="best_overlaps needs"):
        eng.best_overlaps(RL, QID, QS, QE, TID, None, TE, STRAND)
    with pytest.raises(ValueError, match="differ in length"):
        eng.best_overlaps(*HOST_COLS, STRAND[:3])
    with pytest.raises(ValueError, match="one byte per read"):
        eng.best_overlaps(*HOST_COLS, STRAND, skip=SKIP[:2])
    with pytest.raises(TypeError, match="strand as a contiguous uint8"):
        eng.best_overlaps(*DEV_COLS, T(0xB0000, 4, torch.int32))
    with pytest.raises(TypeError, match="skip as a contiguous uint8"):
        eng.best_overlaps(*DEV_COLS, D_STRAND, skip=T(0xC0000, 3, torch.uint8, contiguous=False))
    with pytest.raises(TypeError, match="contiguous int32 CUDA"):
        eng.best_overlaps(D["rl"], T(0x20000, 4, torch.int64), *DEV_COLS[2:], D_STRAND)
    assert side.calls == [] and eng._lib.lib_calls() == []
    assert eng._ctx.value == CTX
