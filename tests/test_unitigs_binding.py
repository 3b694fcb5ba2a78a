"""CPU: the functions of include/raft_hip_utg.h and include/raft_host_utg.h are declared by their bindings (``UTG_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; the summary is eight int64; exports_utg.map names
the three entry points and nothing of the other tables, and libraft_hip_utg.so exports exactly them.  The library is registered under
its tag, in a table that the next library joins without a table of its own.  What ``Engine.unitigs`` hands to the library, against
the recording stand-in of tests/test_binding_calls.py."""
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

CASES = [("raft_hip_utg.h", "raft_hip_", engine), ("raft_host_utg.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_unitigs_device", "raft_hip_unitigs_host", "raft_hip_utg_abi"]
HOST_FUNCTIONS = ["raft_host_write_unitigs"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI", "FLT_ABI", "END_ABI", "BEST_ABI")
SUMMARY = ["reads_in", "reads_skipped", "unitigs", "singletons", "circular", "longest_reads", "longest_length", "total_length"]
RESULT = ["unitig", "index", "offset", "orient", "order", "utg_off", "utg_reads", "utg_length", "utg_circular"]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_utg", "raft_host_utg"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.UTG_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.UTG_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_three_entry_points_and_the_summary():
    assert sorted(header_functions("raft_hip_utg.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.UTG_ABI)
    assert sorted(header_functions("raft_host_utg.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.UTG_ABI)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raft_hip_utg.h")).read(), flags=re.S)
    body = re.search(r"typedef struct raft_hip_utg_summary \{(.*?)\}", text, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
    assert fields == [n for n, _ in engine._UtgSummary._fields_] == SUMMARY
    assert all(t is C.c_int64 for _, t in engine._UtgSummary._fields_) and re.findall(r"\b(\w+)\s+[a-z0-9_]+\s*;", body) == ["int64_t"] * 8
    assert C.sizeof(engine._UtgSummary) == 64
    # the two forms take the same parameters: the context, n_reads, read_len, partner, span, flags, nine outputs, the summary,
    # error_index, the seconds, the launches
    dev, host = (header_functions("raft_hip_utg.h", "raft_hip_")[n] for n in ENTRY_POINTS[:2])
    assert dev == host and len(dev[1]) == 19
    assert engine.UTG_MAX_READS == 2 ** 30 - 1 and "kUtgMaxReads = (1 << 30) - 1" in open(os.path.join(ROOT, "raft_amd", "csrc", "unitig_rule.hpp")).read()


def test_the_library_is_registered_under_its_tag():
    check_side_table("utg", engine.UTG_ABI)
    makefile = open(os.path.join(ROOT, "raft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SIDE \+= utg=unitig_lib$", makefile, flags=re.M)
    assert makefile.index("\nSIDE = ") < makefile.index("\nSIDE += utg=unitig_lib") < makefile.index("\nSIDE_TAGS =") < makefile.index("\nall:")
    host = open(os.path.join(ROOT, "raft_amd", "host", "Makefile")).read()
    # (the CLI links every library of the SIDE list, and both host targets depend on every public header)
    assert "utg" in re.search(r"^SIDE = (.*)$", host, flags=re.M).group(1).split() and "$(SIDE:%=-lraft_hip_%)" in host
    assert "HDRS = $(wildcard ../../include/*.h)" in host and host.count(" $(HDRS)") == 2
    assert all(os.path.exists(os.path.join(ROOT, "include", h)) for h in ("raft_host_utg.h", "raft_hip_utg.h"))


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("utg" in n or "unitig" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and not any("unitig" in n for n in hostio.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())
    assert "unitig" not in open(os.path.join(ROOT, "include", "raft_host.h")).read()
    assert sorted(header_functions("raft_hip_best.h", "raft_hip_")) == sorted(engine.BEST_ABI) and len(engine.BEST_ABI) == 3
    check_side_table("best", engine.BEST_ABI)


def _exported(file):
    path = os.path.join(os.path.dirname(engine._LIB_PATH), file)
    assert os.path.exists(path)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_utg.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    assert os.path.exists(os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_utg.so"))
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    assert _exported("libraft_hip_utg.so") == ENTRY_POINTS
    assert _exported("libraft_hip_best.so") == ["raft_hip_best_abi", "raft_hip_best_overlaps_device", "raft_hip_best_overlaps_host"]


# ---- what Engine.unitigs hands over: three reads
RL = np.array([100, 250, 49], np.int32)
PARTNER, SPAN, FLAGS = np.array([[-1, 1], [0, -1], [-1, -1]], np.int32), np.array([[0, 40], [40, 0], [0, 0]], np.int32), np.array([8, 2, 16], np.uint8)
D_RL, D_PARTNER, D_SPAN, D_FLAGS = T(0x10000, 3), T(0x20000, 6, shape=(3, 2)), T(0x30000, 6), T(0x40000, 3, torch.uint8)
NAMES = {RL.ctypes.data: "rl", PARTNER.ctypes.data: "partner", SPAN.ctypes.data: "span", FLAGS.ctypes.data: "flags",
         D_RL.ptr: "d_rl", D_PARTNER.ptr: "d_partner", D_SPAN.ptr: "d_span", D_FLAGS.ptr: "d_flags"}


def call(monkeypatch, *args):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("utg", side))
    res = eng.unitigs(*args)
    assert len(side.calls) == 1 and eng._lib.lib_calls() == []
    return eng, side.calls[0], res


def check_outputs(res, args, n_reads=3):
    """The nine arrays the library writes are the ones the result holds (cut to what the summary says: the stand-in says nothing)"""
    dtypes = dict(unitig=np.int32, index=np.int32, offset=np.int64, orient=np.uint8, order=np.int32, utg_off=np.int64, utg_reads=np.int32,
                  utg_length=np.int64, utg_circular=np.uint8)
    sizes = dict(unitig=n_reads, index=n_reads, offset=n_reads, orient=n_reads, order=n_reads, utg_off=1, utg_reads=0, utg_length=0, utg_circular=0)
    for key, address in zip(RESULT, args[6:15]):
        assert res[key].dtype == dtypes[key] and res[key].shape == (sizes[key],), key
        assert address != 0 and (res[key].size == 0 or res[key].ctypes.data == address), key
        assert (res[key].base if res[key].base is not None else res[key]).size == n_reads + (1 if key == "utg_off" else 0), key       # sized by n_reads
    assert args[15] == ("_UtgSummary", dict.fromkeys(SUMMARY, 0)) and args[16] == ("i64", -1) and args[17] == ("f64", 0.0) and args[18] == ("i64", 0)
    assert sorted(res) == sorted(RESULT + ["summary", "kernel_seconds", "launches"])
    assert res["summary"] == dict.fromkeys(SUMMARY, 0) and res["kernel_seconds"] == 0.0 and res["launches"] == 0


def test_the_host_form(monkeypatch):
    eng, (name, args), res = call(monkeypatch, RL, PARTNER, SPAN, FLAGS)
    assert name == "raft_hip_unitigs_host" and len(args) == 19
    assert args[:6] == ["ctx", 3, "rl", "partner", "span", "flags"]
    check_outputs(res, args)
    assert eng._lib.calls == []                                       # (no torch stream for host arrays)
    _, (name, args), res = call(monkeypatch, RL, PARTNER.reshape(-1), SPAN.reshape(-1), FLAGS)         # [2n] as well as [n, 2]
    assert name == "raft_hip_unitigs_host" and args[:6] == ["ctx", 3, "rl", "partner", "span", "flags"]
    check_outputs(res, args)


def test_the_device_form(monkeypatch):
    eng, (name, args), res = call(monkeypatch, D_RL, D_PARTNER, D_SPAN, D_FLAGS)
    assert name == "raft_hip_unitigs_device" and len(args) == 19
    assert args[:6] == ["ctx", 3, "d_rl", "d_partner", "d_span", "d_flags"]
    check_outputs(res, args)
    assert eng._lib.calls == [("use_torch_stream", [])]
    assert eng.last_unitigs_launches == 0 and eng.last_unitigs_seconds == 0.0


def test_no_reads(monkeypatch):
    empty = np.zeros(0, np.int32)
    _, (name, args), res = call(monkeypatch, empty, np.zeros((0, 2), np.int32), empty, np.zeros(0, np.uint8))
    assert name == "raft_hip_unitigs_host" and args[:6] == ["ctx", 0, 0, 0, 0, 0]
    assert res["unitig"].shape == (0,) and res["utg_off"].shape == (1,) and res["order"].shape == (0,)


def test_what_is_refused_before_any_call(monkeypatch):
    eng = make_engine(NAMES)
    side = Lib(NAMES)
    monkeypatch.setattr(engine, "load_side_library", side_library("utg", side))
    with pytest.raises(ValueError, match="unitigs needs read_len, partner, span and flags"):
        eng.unitigs(RL, PARTNER, SPAN, None)
    with pytest.raises(ValueError, match="unitigs needs"):
        eng.unitigs(RL, None, SPAN, FLAGS)
    with pytest.raises(ValueError, match="two values per read"):
        eng.unitigs(RL, PARTNER[:2], SPAN, FLAGS)
    with pytest.raises(ValueError, match="two values per read"):
        eng.unitigs(RL, PARTNER, SPAN.reshape(-1)[:5], FLAGS)
    with pytest.raises(ValueError, match="flags one byte"):
        eng.unitigs(RL, PARTNER, SPAN, FLAGS[:2])
    with pytest.raises(TypeError, match="flags as a contiguous uint8"):
        eng.unitigs(D_RL, D_PARTNER, D_SPAN, T(0x40000, 3, torch.int32))
    with pytest.raises(TypeError, match="flags as a contiguous uint8"):
        eng.unitigs(D_RL, D_PARTNER, D_SPAN, T(0x40000, 3, torch.uint8, contiguous=False))
    with pytest.raises(TypeError, match="contiguous int32 CUDA"):
        eng.unitigs(D_RL, T(0x20000, 6, torch.int64), D_SPAN, D_FLAGS)
    assert side.calls == [] and eng._lib.lib_calls() == []
    assert eng._ctx.value == CTX
